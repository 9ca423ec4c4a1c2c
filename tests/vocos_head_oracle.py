"""The Vocos head in float64 (promonet/model/vocos.py:163-206), the case
tables of tests/test_gpu_vocos_head.py, the figure they are compared by and
the gates. Not a test: the oracle of test_cpu_vocos_head.py and
test_gpu_vocos_head.py. It shares no code with promonet_amd.

Everything works in float64 on the exact values of the fp32 inputs:

  frames       irfft at n = 1024, norm='backward', times the window
  overlap_add  fold in frame order at hop 256, divided by the window^2
               envelope of the frames that exist, 384 samples cropped at each
               end
  head         mag = min(exp(l), 100), spec = mag e^{i phi}, then the two above

`defect` plants one wrong reading (DEFECTS); test_cpu_vocos_head.py shows that
the comparisons of the GPU tests reject each of them.

Three tables, each the smallest that reaches every index:

  per bin  (the spectrum entry, pm_istft) one bin alone in every fourth frame,
           every other frame zero: a sample receives one live frame, so each
           of the 513 bins is judged alone over its own 1024 samples
  exact    only bins 0 and 512, integers, a window of m / 64: every operation
           of the transform and of the fold is exact in fp32 but the last
           division, which fp32 rounds correctly; held with torch.equal
  head     (the logits entry, pm_vocos_head) one-hot activations, so that a
           column of head.out.weight IS the logits of a frame, exactly, in
           every operand type; -128 silences all bins but one

The figure of a frame is max |got - want| over the samples the frame reaches,
over the RMS of want over the same samples; a case's figure is the largest
over its live frames. The gate is 4 x the figure of the reference's own fp32
arithmetic (torch.exp, clip, cos, sin, torch.fft.irfft, the window and the
fold of vocos_oracle.istft) on the same table against the same oracle: this
project's margin for one more rounding order.
"""
import torch

import vocos_oracle

N_FFT = 1024
HOP = 256
BINS = N_FFT // 2 + 1
PAD = (N_FFT - HOP) // 2
CHANNELS = 512
CLIP = 100.

DEFECTS = (
    'imag_dc_kept', 'imag_nyquist_kept', 'image_not_conjugated',
    'window_mirrored', 'crop_383', 'envelope_unclamped', 'clip_before_exp',
    'clip_at_10')


###############################################################################
# The oracle
###############################################################################


def frames(spec, window, defect=None):
    """complex (B, 513, T), window (1024) -> float64 (B, T, 1024): the
    windowed inverse real transform of every frame. The imaginary parts of
    bins 0 and 512 play no part, as in a C2R transform."""
    assert defect is None or defect in DEFECTS
    spec = spec.to(torch.complex128).clone()
    window = window.to(torch.float64)
    real, imag = spec.real.clone(), spec.imag.clone()
    # A transform that packs the 513 bins into 512 complex points has
    # Z[0] = (X[0] + X[512]) / 2 + i (X[0] - X[512]) / 2 for real X[0] and
    # X[512]. An imaginary part left in either is read as the OTHER bin's real
    # part, negated
    if defect == 'imag_dc_kept':
        real[:, BINS - 1] -= imag[:, 0]
    if defect == 'imag_nyquist_kept':
        real[:, 0] -= imag[:, BINS - 1]
    # X[1024 - k] = X[k], not its conjugate: the sines cancel
    if defect == 'image_not_conjugated':
        imag[:, 1:BINS - 1] = 0.
    imag[:, 0] = 0.
    imag[:, BINS - 1] = 0.
    signal = torch.fft.irfft(
        torch.complex(real, imag), N_FFT, dim=1, norm='backward')
    if defect == 'window_mirrored':
        window = window.flip(0)
    return (signal * window[None, :, None]).transpose(1, 2).contiguous()


def overlap_add(windowed, window, defect=None):
    """float64 (B, T, 1024) -> (B, 256 T)"""
    assert defect is None or defect in DEFECTS
    batch, count, _ = windowed.shape
    length = (count - 1) * HOP + N_FFT
    square = window.to(torch.float64).square()
    y = torch.zeros(batch, length, dtype=torch.float64)
    envelope = torch.zeros(length + N_FFT, dtype=torch.float64)
    for t in range(count):                          # fold: frame order
        y[:, t * HOP:t * HOP + N_FFT] += windowed[:, t]
        envelope[t * HOP:t * HOP + N_FFT] += square
    if defect == 'envelope_unclamped':
        # frames T, T + 1, T + 2 do not exist, but reach below 256 T + 384
        for t in range(count, count + 3):
            envelope[t * HOP:t * HOP + N_FFT] += square
    crop = PAD - 1 if defect == 'crop_383' else PAD
    return (y / envelope[:length])[:, crop:crop + count * HOP]


def istft(spec, window, defect=None):
    return overlap_add(frames(spec, window, defect), window, defect)


def spectrum(logits, defect=None):
    """fp32 logits (B, T, 1026) -> complex128 (B, 513, T)"""
    assert defect is None or defect in DEFECTS
    logits = logits.to(torch.float64)
    log_magnitude, phase = logits[..., :BINS], logits[..., BINS:]
    if defect == 'clip_before_exp':
        magnitude = torch.exp(log_magnitude.clamp(max=CLIP))
    elif defect == 'clip_at_10':
        magnitude = torch.exp(log_magnitude).clamp(max=10.)
    else:
        magnitude = torch.exp(log_magnitude).clamp(max=CLIP)
    return torch.polar(magnitude, phase).transpose(1, 2)


def head(logits, window, defect=None):
    """fp32 logits (B, T, 1026): log-magnitude [0, 513) | phase [513, 1026)
    -> float64 (B, 256 T)"""
    return istft(spectrum(logits, defect), window, defect)


###############################################################################
# The reference's own arithmetic in fp32: the yardstick of the gates
###############################################################################


def reference_istft(spec, window):
    return vocos_oracle.istft(spec.to(torch.complex64), window.float())


def reference_head(logits, window):
    log_magnitude, phase = logits.float().transpose(1, 2).chunk(2, dim=1)
    magnitude = torch.clip(torch.exp(log_magnitude), max=1e2)
    spec = magnitude * (torch.cos(phase) + 1j * torch.sin(phase))
    return vocos_oracle.istft(spec, window.float())


###############################################################################
# The figure
###############################################################################


def span(frame, count):
    """The samples [first, last) of the cropped output that a frame reaches"""
    return (max(0, frame * HOP - PAD),
            min(count * HOP, frame * HOP - PAD + N_FFT))


def figure(got, want, live):
    """(worst figure, the entry of `live` it belongs to). got, want
    (B, 256 T); live: [(row, frame, ...)], frames that share no sample with
    another live frame."""
    got = torch.as_tensor(got).to(torch.float64)
    count = want.shape[1] // HOP
    worst, where = -1., None
    for entry in live:
        row, frame = entry[:2]
        first, last = span(frame, count)
        target = want[row, first:last]
        value = ((got[row, first:last] - target).abs().max() /
                 target.square().mean().sqrt()).item()
        if not value <= worst:                      # NaN is the worst
            worst, where = value, entry
        if value != value:
            break
    return worst, where


###############################################################################
# The per-bin table (the spectrum entry)
###############################################################################


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def per_bin_table():
    """(spec complex64 (2, 513, 2056), window (1024), live [(row, frame,
    bin)]): frame 4 m of row 0 holds bin m alone, of row 1 bin 512 - m; its
    value is (a, b), |a| and |b| in [0.5, 2], also at bins 0 and 512. The
    window is not Hann (and nonzero where the envelope is)."""
    def make():
        generator = torch.Generator().manual_seed(513)
        count = 4 * BINS + 4
        size = torch.rand(2, 2, BINS, generator=generator) * 1.5 + .5
        sign = torch.randint(0, 2, (2, 2, BINS), generator=generator) * 2 - 1
        value = size * sign
        spec = torch.zeros(2, BINS, count, dtype=torch.complex64)
        live = []
        for row in range(2):
            for m in range(BINS):
                k = m if row == 0 else BINS - 1 - m
                spec[row, k, 4 * m] = complex(value[row, 0, m],
                                              value[row, 1, m])
                live.append((row, 4 * m, k))
        window = torch.hann_window(N_FFT) * (
            1 + .3 * torch.rand(N_FFT, generator=generator)) + .01
        return spec, window, live
    return _once('per bin', make)


def per_bin_oracle():
    return _once('per bin oracle', lambda: istft(*per_bin_table()[:2]))


def per_bin_fp32_figure():
    spec, window, live = per_bin_table()
    return figure(reference_istft(spec, window), per_bin_oracle(), live)[0]


###############################################################################
# The exact table (the spectrum entry)
###############################################################################


EXACT_FRAMES = (1, 2, 3, 4, 5, 9)
EXACT_BATCH = 3


def exact_window():
    """m / 64, m an integer in [1, 64]: not symmetric"""
    generator = torch.Generator().manual_seed(64)
    return torch.randint(1, 65, (N_FFT,), generator=generator).float() / 64.


def exact_table(count):
    """(spec complex64 (3, 513, count), window): integers in [-8, 8] at the
    real parts of bins 0 and 512 and nothing else, but for their imaginary
    parts, which are nonzero and must be dropped.

    Why fp32 is exact here. A frame's sample n is (X[0] + (-1)^n X[512]) /
    1024 times m / 64, an integer of magnitude <= 16 x 64 in units of 2^-16.
    A packed transform sees Z[0] = ((X[0] + X[512]) / 2, (X[0] - X[512]) / 2)
    and zeros: every butterfly adds a zero, and the scale is a power of two.
    A sum of at most four samples stays below 2^12 units, a sum of at most
    four m^2 / 4096 below 2^14 units of 2^-12: both exact in any order, with
    or without fused multiply-adds. The one inexact operation is the final
    division; fp32 division is correctly rounded, and so is a float64
    quotient of two fp32 values rounded to fp32 (53 >= 2 x 24 + 2 bits).
    Hence the oracle rounded ONCE to fp32 is the only right answer."""
    generator = torch.Generator().manual_seed(100 + count)
    shape = (EXACT_BATCH, 2, count)
    # 3 t and 7 t step through all residues of 17: every frame and every row
    # has values of its own
    t = torch.arange(count)[None]
    row = torch.arange(EXACT_BATCH)[:, None]
    real = torch.stack([(3 * t + 5 * row + 1) % 17 - 8,
                        (7 * t + 11 * row + 4) % 17 - 8], dim=1).float()
    imag = torch.randint(1, 6, shape, generator=generator).float() * (
        torch.randint(0, 2, shape, generator=generator) * 2 - 1)
    spec = torch.zeros(EXACT_BATCH, BINS, count, dtype=torch.complex64)
    spec[:, 0] = torch.complex(real[:, 0], imag[:, 0])
    spec[:, BINS - 1] = torch.complex(real[:, 1], imag[:, 1])
    return spec, exact_window()


def exact_oracle(count, defect=None):
    """fp32 (3, 256 count): the float64 oracle rounded once"""
    return istft(*exact_table(count), defect).to(torch.float32)


###############################################################################
# The head table (the logits entry)
###############################################################################


HEAD_SETS = ('low', 'high')
SILENT = -128.                  # expf(-128) is exactly 0 in fp32
SILENT_CHANNEL = CHANNELS - 1
LIVE_CHANNELS = CHANNELS - 1
HEAD_FRAMES = 4 * LIVE_CHANNELS + 4
# multiples of 1/4 in [-6, 6], and 4.625: e^4.5 = 90.02 is below the clip,
# e^4.625 = 102.0 and e^5 = 148.4 are clipped to exactly 100
LOG_MAGNITUDES = tuple(i / 4. for i in range(-24, 25)) + (4.625,)
CLIP_SIDES = (4.5, 4.625, 5.)
LARGE_PHASES = (1000., -996., -1000., 996.)


def head_bin(which, channel):
    """The bin that a live channel sounds: 'low' 0 .. 510, 'high' 512 .. 2"""
    return channel if which == 'low' else BINS - 1 - channel


def head_log_magnitude(which, channel):
    shift = 0 if which == 'low' else 23
    return LOG_MAGNITUDES[(7 * channel + shift) % len(LOG_MAGNITUDES)]


def head_weight(which):
    """head.out.weight (1026, 512): column c is the logit pattern of channel
    c. Every value has at most 8 significant bits: exact as an fp32, f16 or
    bf16 operand."""
    channel = torch.arange(CHANNELS)[None]
    k = torch.arange(BINS)[:, None]
    # phases k / 8, 0 < |k| < 256, at every bin, the silent ones too
    eighths = (5 * k + 3 * channel + (0 if which == 'low' else 101)) % 509 \
        - 254
    eighths[eighths == 0] = 1
    phase = eighths.float() / 8.
    log_magnitude = torch.full((BINS, CHANNELS), SILENT)
    for c in range(LIVE_CHANNELS):
        own = head_bin(which, c)
        log_magnitude[own, c] = head_log_magnitude(which, c)
        if c % 16 == 3:
            phase[own, c] = LARGE_PHASES[(c // 16) % 4]
    return torch.cat([log_magnitude, phase]).contiguous()


def head_table(which):
    """(x one-hot (2, 2048, 512), weight (1026, 512), window (1024), live
    [(row, frame, channel, bin, log-magnitude)]). Frame 4 m of row 0 is
    channel m, of row 1 channel 510 - m; every other frame is the all-silent
    channel 511. The bias is zero and the window the periodic Hann window of
    the checkpoint."""
    def make():
        weight = head_weight(which)
        x = torch.zeros(2, HEAD_FRAMES, CHANNELS)
        x[:, :, SILENT_CHANNEL] = 1.
        live = []
        for row in range(2):
            for m in range(LIVE_CHANNELS):
                c = m if row == 0 else LIVE_CHANNELS - 1 - m
                x[row, 4 * m, SILENT_CHANNEL] = 0.
                x[row, 4 * m, c] = 1.
                live.append((row, 4 * m, c, head_bin(which, c),
                             head_log_magnitude(which, c)))
        return x, weight, torch.hann_window(N_FFT), live
    return _once(('head', which), make)


def head_logits(which):
    """(2, 2048, 1026) fp32, exact: a row of x selects a column of weight"""
    x, weight, _, _ = head_table(which)
    return (x.double() @ weight.double().T).float()


def head_oracle(which, defect=None):
    def make():
        return head(head_logits(which), head_table(which)[2], defect)
    return _once(('head oracle', which, defect), make)


def head_silence(which):
    """The first sample of the cropped output that only all-silent frames
    reach: from there on the audio is exactly zero"""
    return span(4 * (LIVE_CHANNELS - 1), HEAD_FRAMES)[1]


def head_fp32_figure():
    worst = 0.
    for which in HEAD_SETS:
        _, _, window, live = head_table(which)
        got = reference_head(head_logits(which), window)
        worst = max(worst, figure(got, head_oracle(which), live)[0])
    return worst


###############################################################################
# The gates
###############################################################################


# The figures of the reference's fp32 arithmetic on the two tables.
# torch.fft.irfft runs MKL's transform on the CPU, and MKL picks its code by
# the processor; the recorded figures are those of the path that every x86-64
# processor can take, which MKL_CBWR=COMPATIBLE reproduces on any machine
# (test_cpu_vocos_head.py holds them to these digits in a child process).
PER_BIN_FP32_FIGURE = 1.043e-06     # 1.045e-06 on MKL's AVX-512 path
HEAD_FP32_FIGURE = 1.029e-06        # 8.788e-07
PER_BIN_GATE = 4 * PER_BIN_FP32_FIGURE
HEAD_GATE = 4 * HEAD_FP32_FIGURE

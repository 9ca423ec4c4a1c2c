"""Oracle of the preprocessing transforms (spectrogram.from_audio, its log-mel,
loudness.from_audio): float64 truth, an fp32 error model per output, the case
table, and a float64 model of the kernel's algebra that takes planted defects.

TRUTH is the contract in float64 with unrounded tables, as oracle/restatement.py
states it (`spectrogram`, `linear_to_mel`, `loudness`, `band_average`): reflect
pad 384, periodic Hann 1024, hop 256, T = N // 256, |X| per bin.

ERROR MODEL. A float32 transform of 1024 points carries, per frame,

    delta_k = 2^-24 * 10 * ||w x||_2 + 2^-23 * |X_k|

into bin k (the harmonics STFT's model with log2(1024) = 10), and every
epilogue passes it on by its Lipschitz constant:

    magnitude sqrt(X^2 + 1e-6)  (|X| delta + delta^2 / 2) / out + 2^-23 out
    dB per bin                  (20 / ln 10) delta / max(|X|, 1e-5) + 2^-22 |v|
    band mean                   mean of its bins' bounds + 2^-22 |mean|
    log-mel                     sum_f b_f bound_f / sum_f b_f out_f
                                + span 2^-24 + 2^-22 |log|

The floor max - 80, the 1e-10 clamp and the MIN_DB clamp are 1-Lipschitz: no
bin is left out. A frame that sees the floor takes the larger of its own bound
and the bound of the utterance's maximum bin (the floor moves with that bin).
A FIGURE is the largest error divided by its bound.

GATES. A family's gate is K x model with K = 4 x the largest figure that
torch's own fp32 evaluation of the contract (torch.stft in fp32 with the fp32
window, then the reference's torch ops, on the CPU) reaches on the case table.
The figures are recorded in GATES and held by tests/test_cpu_preprocess_bins.py
to 2 %, in a child process on the code path every x86-64 processor has
(MKL_CBWR=COMPATIBLE, one thread), as tests/harmonics_oracle.py does: MKL
chooses its transform by the processor, and the figures move with it (the
clean cosines' magnitude: 2.66 on an AVX-512 path, 15.52 on the common one,
whose error in the empty bins is 4 x delta - squared under sqrt(X^2 + 1e-6)).
numpy.fft.rfft is no yardstick: it computes float32 input in double.
(restatement.loudness returns float32: the dB truth carries that rounding,
2^-24 |v|, a quarter of the bound's last term.)
"""
import functools
import math

import numpy as np
import torch

import restatement as R

NFFT, HOP, PAD, BINS = 1024, 256, 384, 513
MIN_DB, TOP_DB = R.MIN_DB, 80.
U24, U23, U22 = 2. ** -24, 2. ** -23, 2. ** -22
DB = 20. / math.log(10.)
FAMILIES = ('magnitude', 'log_mel', 'db_bin', 'band_mean')

# The largest figure of torch's fp32 evaluation per family over `cases()`
# (fp32_figures; the case that sets each: test_cpu_preprocess_bins.py prints
# them all). K = 4 x.
GATES = {
    'magnitude': 15.519,    # cosines: an empty bin
    'log_mel': 3.821,       # cosines
    'db_bin': 3.886,        # frames_35
    'band_mean': 0.416,     # impulses
}
K = {family: 4. * figure for family, figure in GATES.items()}

# the flat gates of SURVEY 8(d) that the older tests hold (for the blind-spot
# statement of test_cpu_preprocess_bins.py only)
OLD_STFT_GATE = (2e-5, 1e-5)
OLD_LOUDNESS_GATE = (1e-4, 1e-5)


###############################################################################
# Truth and the error models
###############################################################################


def truth(audio):
    """audio (B, N) -> dict of float64 tensors: `magnitude` (B, 513, T),
    `x` = |X|, `l2` = ||w x||_2 per frame (B, 1, T, by Parseval), `log_mel`
    (B, 80, T), `db` (B, 513, T) = the per-bin loudness, `raw_db` = 20 log10
    max(1e-5, |X|) and `floor` (B, 1, 1) = each utterance's max - 80."""
    audio = audio.double()
    batch = audio.shape[0]
    magnitude = R.spectrogram(audio[:, None]).reshape(batch, BINS, -1)
    power = (magnitude ** 2 - 1e-6).clamp_min(0.)
    x = power.sqrt()
    full = power[:, :1] + power[:, -1:] + 2. * power[:, 1:-1].sum(1, True)
    l2 = (full / NFFT).sqrt()
    db = torch.stack([
        R.loudness(audio[row:row + 1], None).double()
        for row in range(batch)])
    raw = DB * torch.log(x.clamp_min(1e-5))
    return {
        'magnitude': magnitude, 'x': x, 'l2': l2,
        'log_mel': R.linear_to_mel(magnitude), 'db': db, 'raw_db': raw,
        'floor': raw.amax((1, 2), True) - TOP_DB}


def delta(t):
    return U24 * 10. * t['l2'] + U23 * t['x']


def magnitude_bound(t):
    d, out = delta(t), t['magnitude']
    return (t['x'] * d + d * d / 2.) / out + U23 * out


def db_bound(t, value=None):
    """Per bin (B, 513, T); `value` defaults to the truth's."""
    value = t['db'] if value is None else value
    own = DB * delta(t) / t['x'].clamp_min(1e-5)
    # the utterance's maximum bin carries the floor
    flat = t['raw_db'].flatten(1).argmax(1)
    top = torch.stack([own[row].flatten()[flat[row]]
                       for row in range(own.shape[0])])[:, None, None]
    sees = t['raw_db'].amin(1, True) <= t['floor'] + 1e-2
    own = torch.where(sees, torch.maximum(own, top), own)
    return own + U22 * value.abs()


def band_edges(bands):
    if bands == 1:
        return [0, BINS]
    step = BINS / bands
    return [int(b * step) for b in range(bands)] + [int(bands * step)]


def band_bound(t, bands):
    per_bin = db_bound(t)
    edges = band_edges(bands)
    rows = [per_bin[:, lo:hi].mean(1) for lo, hi in zip(edges, edges[1:])]
    return torch.stack(rows, 1) + U22 * R.band_average(t['db'], bands).abs()


def mel_bound(t, basis=None, log_mel=None):
    """(B, M, T); where the truth is -inf (an all-zero filter) the bound is
    0: the value is -inf, or the clamp's threshold, exactly."""
    basis = (R.mel_basis() if basis is None else basis).double()
    log_mel = t['log_mel'] if log_mel is None else log_mel
    span = spans(basis)
    length = torch.tensor(
        [hi - lo for lo, hi, _ in span], dtype=torch.float64)[None, :, None]
    up = torch.matmul(basis, magnitude_bound(t))
    down = torch.matmul(basis, t['magnitude'])
    bound = up / down + length * U24 + U22 * log_mel.abs()
    return torch.where(torch.isfinite(log_mel), bound,
                       torch.zeros_like(bound))


def spans(basis):
    """(lo, hi, offset) per filter as pm_mel_csr_kernel lays them out: first
    and one-past-last non-zero column (0, 0 for an all-zero row), and the
    offset of the span among the compacted values."""
    out, total = [], 0
    for row in basis:
        nz = torch.nonzero(row).flatten()
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
        out.append((lo, hi, total))
        total += hi - lo
    return out


def compacted(basis):
    return torch.cat([basis[m, lo:hi] for m, (lo, hi, _) in
                      enumerate(spans(basis))] + [basis.new_zeros(0)])


def figure(got, want, bound):
    """Largest error over its bound; where the truth is infinite (an empty
    mel filter) the value must be that infinity."""
    got, want = got.double().cpu(), want.double()
    finite = torch.isfinite(want)
    if not finite.all():
        assert torch.equal(got[~finite], want[~finite])
    if not finite.any():
        return 0.
    error = (got - want)[finite].abs()
    ratio = torch.where(error == 0., error, error / bound[finite])
    assert not ratio.isnan().any()
    return ratio.max().item()


def figures(t, magnitude=None, log_mel=None, db=None, bands=None):
    """The figures of whatever evaluation is given, by family"""
    out = {}
    if magnitude is not None:
        out['magnitude'] = figure(magnitude, t['magnitude'], magnitude_bound(t))
    if log_mel is not None:
        out['log_mel'] = figure(log_mel, t['log_mel'], mel_bound(t))
    if db is not None:
        out['db_bin'] = figure(db, t['db'], db_bound(t))
    if bands is not None:
        out['band_mean'] = max(
            figure(got, R.band_average(t['db'], n), band_bound(t, n))
            for n, got in bands.items())
    return out


###############################################################################
# torch's fp32 evaluation of the contract: the yardstick
###############################################################################


def fp32(audio):
    """torch.stft in fp32 with the fp32 window, then the reference's torch ops
    in fp32 on the CPU. audio (B, N) float32."""
    audio = audio.float()
    batch = audio.shape[0]
    magnitude = R.spectrogram(audio[:, None]).reshape(batch, BINS, -1)
    log_mel = R.linear_to_mel(magnitude)
    window = torch.hann_window(NFFT, dtype=torch.float32)
    padded = torch.nn.functional.pad(audio[:, None], (PAD, PAD), 'reflect')
    stft = torch.stft(
        padded[:, 0], NFFT, hop_length=HOP, window=window, center=False,
        return_complex=True)
    # librosa.amplitude_to_db on |S| (restatement.loudness), in fp32
    power = stft.abs().square()
    db = 10. * torch.log10(power.clamp_min(1e-10))
    db = torch.maximum(db, db.amax((1, 2), True) - TOP_DB)
    weights = torch.from_numpy(R.perceptual_weights()).float()
    db = (db + weights).clamp_min(MIN_DB)
    return {'magnitude': magnitude, 'log_mel': log_mel, 'db': db}


def fp32_figures(name):
    """{family: figure} of torch's fp32 evaluation on one case"""
    audio = cases()[name]
    got, t = fp32(audio), case_truth(name)
    return figures(
        t, got['magnitude'], got['log_mel'], got['db'],
        {n: R.band_average(got['db'], n) for n in (8, 1, 5)})


###############################################################################
# The case table
###############################################################################

COSINE_BINS = (0, 1, 63, 64, 255, 256, 257, 320, 384, 448, 511, 512)
# both reflections of cos(2 pi k n / 1024) are the cosine itself when the last
# sample sits at a multiple of 1024: every frame keeps exactly bins k - 1, k,
# k + 1 (and the odd length puts every second row on the unaligned load)
COSINE_SAMPLES = 2049
# per-bin rms of the noise under the cosine's peak bin: by the oracle a
# quarter of the dB bins then sit on the max - 80 floor
FLOOR_NOISE_DB = -75.
LENGTHS = (385, 511, 512, 640, 1023, 1024, 1151, 1152, 1153)
# (18 and 34 leave a last group of 2 frames: nf % 4 = 2 at both group sizes)
FRAME_COUNTS = (1, 3, 15, 16, 17, 18, 31, 32, 33, 34, 35)
WINDOW_L2 = math.sqrt(384.)            # ||hann||_2


def cosines(dtype=torch.float32, bins=COSINE_BINS, samples=COSINE_SAMPLES):
    n = torch.arange(samples, dtype=torch.float64)
    k = torch.tensor(bins, dtype=torch.float64)[:, None]
    return (.5 * torch.cos(2. * math.pi * k * n / NFFT)).to(dtype)


def floor_noise(rows, samples, peak, seed, level=FLOOR_NOISE_DB):
    """White noise whose bins have rms `level` dB under `peak` (per row)"""
    noise = torch.randn(
        rows, samples, generator=torch.Generator().manual_seed(seed),
        dtype=torch.float64)
    sigma = torch.as_tensor(peak, dtype=torch.float64).reshape(-1, 1) * \
        10. ** (level / 20.) / WINDOW_L2
    return noise * sigma


def cosines_over_floor(bins=COSINE_BINS, samples=COSINE_SAMPLES, seed=7,
                       scale=None):
    clean = cosines(torch.float64, bins, samples)
    # peak bin: A / 2 * sum(w) = 128, twice that where k pairs with itself
    peak = torch.tensor([256. if k in (0, 512) else 128. for k in bins])
    audio = clean + floor_noise(len(bins), samples, peak, seed)
    if scale is not None:
        audio = audio * torch.as_tensor(scale, dtype=torch.float64)[:, None]
    return audio.float()


def impulses():
    """One unit sample a row: in the left reflection (frame 0 sees it
    twice), on sample 0 (reflected onto itself: seen once), in the interior,
    in the right reflection and on the last sample."""
    samples = 2048
    audio = torch.zeros(5, samples)
    for row, position in enumerate(IMPULSE_POSITIONS):
        audio[row, position] = 1.
    return audio


IMPULSE_POSITIONS = (300, 0, 1001, 1748, 2047)


def noise(rows, samples, seed, amplitude=.1):
    return torch.randn(
        rows, samples, generator=torch.Generator().manual_seed(seed)) * amplitude


def levels():
    """Silence, noise under the 1e-5 amplitude clamp, a full-scale square
    wave, a loud row beside one 60 dB quieter, DC + Nyquist + noise: every
    row keeps its own floor."""
    samples = 7 * 256 + 77
    n = torch.arange(samples)
    audio = torch.zeros(6, samples)
    audio[1] = (torch.rand(
        samples, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 1e-6
    audio[2] = torch.where((n // 32) % 2 == 0, 1., -1.)
    audio[3] = noise(1, samples, 4, .3)[0]
    audio[4] = audio[3] * 1e-3
    audio[5] = .3 + .2 * (-1.) ** n + noise(1, samples, 5, 1e-3)[0]
    return audio


def lengths_case(samples):
    """B = 3 at one of LENGTHS: a cosine over its floor, noise, and noise
    40 dB down"""
    audio = noise(3, samples, 100 + samples)
    audio[0] = cosines_over_floor((64,), samples, seed=samples)[0]
    audio[2] *= .01
    return audio


def frames_case(frames):
    """B = 2 at T = frames (N % 256 = 129, T = 1 at the shortest input there
    is): cosines over their floors at two levels"""
    return cosines_over_floor(
        (320, 1), frames * HOP + 129, seed=200 + frames, scale=(1., .05))


def floor_decision(side):
    """An utterance whose first 16-frame group is silent - every dB bin on the
    1e-10 clamp, -100 dB exactly - under a bin-centred cosine whose peak bin
    sits at -20 dB + side x 5e-4 dB: the utterance's floor lies 5e-4 dB above
    (side = +1: the group's minimum is under the floor) or below (-1: it is
    not) that group's minimum."""
    samples = 48 * HOP
    amplitude = 10. ** ((-20. + side * 5e-4) / 20.) / 256.     # |X_64| / 256
    n = torch.arange(samples, dtype=torch.float64)
    audio = amplitude * torch.cos(2. * math.pi * 64. * n / NFFT)
    audio[:24 * HOP] = 0.
    return audio.float()[None]


def walk_case(grid, frames_per_group=16, rows=5):
    """The smallest batch of `rows` utterances whose groups exceed `grid`
    workgroups by a handful, the per-row group count no multiple of 8:
    cosine-over-floor rows at different levels. Returns (audio, groups)."""
    groups = grid // rows + 1
    while groups % 8 == 0 or groups * rows <= grid:
        groups += 1
    frames = groups * frames_per_group - 5
    bins = (64, 320, 448, 1, 511, 257, 384, 63)[:rows]
    scale = [10. ** (-row / 2.) for row in range(rows)]
    return cosines_over_floor(
        bins, frames * HOP + 77, seed=300, scale=scale), groups


@functools.lru_cache(maxsize=None)
def cases():
    """name -> audio (B, N) float32. Built once; nobody writes to them."""
    out = {
        'noise': noise(2, 8 * HOP + 77, 1),
        'impulses': impulses(),
        'cosines': cosines(),
        'cosines_floor': cosines_over_floor(),
        'levels': levels(),
        'floor_above': floor_decision(+1),
        'floor_below': floor_decision(-1),
    }
    for samples in LENGTHS:
        out[f'length_{samples}'] = lengths_case(samples)
    for frames in FRAME_COUNTS:
        out[f'frames_{frames}'] = frames_case(frames)
    return out


@functools.lru_cache(maxsize=None)
def case_truth(name):
    return truth(cases()[name])


def floor_shares(t):
    """(share of the dB bins on the max - 80 floor, share above it)"""
    under = (t['raw_db'] < t['floor']).double().mean().item()
    return under, 1. - under


###############################################################################
# The kernel's algebra in float64, with planted defects
###############################################################################
# pm_fft.h: the 1024 windowed samples packed into 512 complex points z[n] =
# x[2 n] + i x[2 n + 1], Z = DFT512(z) out of the W512 table, and bins k and
# 512 - k unpacked from the pair (Z[k], Z[512 - k]) with the W1024 table:
#     2 X[k] = E - i W1024^k D,  E = Z[k] + conj Z[512 - k], D = Z[k] - conj ..
# bins 0 and 512 = Re Z[0] +- Im Z[0], bin 256 = conj-free |Z[256]|. With no
# defect this equals the truth to 1e-12 (test_cpu_preprocess_bins.py).

DEFECTS = (
    'window_2e-6', 'w1024_2e-6', 'w512_entry', 'symmetric_left',
    'symmetric_right', 'exchange_lane', 'dc_nyquist_signs', 'bin256_doubled',
    'lane0_bands', 'bin512_left_out', 'band7_by_64', 'floor_of_neighbour',
    'floor_after_weights', 'mel_span_short_lo', 'mel_span_short_hi',
    'mel_offset_shifted')


def model_tables(defect=None):
    n = np.arange(NFFT)
    hann = .5 - .5 * np.cos(2. * np.pi * n / NFFT)
    w512 = np.exp(-2j * np.pi * np.arange(512) / 512.)
    w1024 = np.exp(-2j * np.pi * np.arange(513) / 1024.)
    if defect == 'window_2e-6':
        # (what a fast-math cosine gives: each entry off, not a common scale)
        sign = np.where(np.random.RandomState(0).rand(NFFT) < .5, -1., 1.)
        hann = hann * (1. + 2e-6 * sign)
    if defect == 'w1024_2e-6':
        sign = np.where(np.random.RandomState(1).rand(513) < .5, -1., 1.)
        w1024 = w1024 * (1. + 2e-6 * sign)
    if defect == 'w512_entry':
        w512[0] += 2. ** -20
    return hann, w512, w1024


def model_frames(audio, left='reflect', right='reflect'):
    """(B, N) float64 numpy -> (B, T, 1024) padded frames"""
    samples = audio.shape[-1]
    frames = samples // HOP
    index = np.arange(frames)[:, None] * HOP + np.arange(NFFT)[None] - PAD
    low = -index if left == 'reflect' else -index - 1
    index = np.where(index < 0, low, index)
    high = 2 * (samples - 1) - index if right == 'reflect' else \
        2 * samples - 1 - index
    index = np.where(index >= samples, high, index)
    return audio[:, index]


def model_bins(audio, defect=None):
    """|X| (B, 513, T) in float64 by the kernel's algebra"""
    audio = np.asarray(audio, dtype=np.float64)
    hann, w512, w1024 = model_tables(defect)
    frames = model_frames(
        audio, 'symmetric' if defect == 'symmetric_left' else 'reflect',
        'symmetric' if defect == 'symmetric_right' else 'reflect') * hann
    z = frames[..., 0::2] + 1j * frames[..., 1::2]
    j = np.arange(512)
    big = z @ w512[np.outer(j, j) % 512]
    k = np.arange(513)
    zk, zm = big[..., k % 512], np.conj(big[..., (512 - k) % 512])
    e, d = zk + zm, zk - zm
    x = .5 * (e - 1j * w1024 * d)
    if defect == 'dc_nyquist_signs':
        x[..., 0] = big[..., 0].real - big[..., 0].imag
        x[..., 512] = big[..., 0].real + big[..., 0].imag
    x = np.abs(x)
    if defect == 'exchange_lane':
        # one lane (17) writes its bins k and 512 - k to each other's places
        for q in range(4):
            lo, hi = 17 + 64 * q, 512 - 17 - 64 * q
            x[..., [lo, hi]] = x[..., [hi, lo]]
    if defect == 'bin256_doubled':
        x[..., 256] *= 2.
    return torch.from_numpy(np.swapaxes(x, 1, 2).copy())


def model_outputs(audio, defect=None):
    """The kernel's outputs in float64: magnitude, log-mel, dB per bin and
    the 8 band means, by the same steps as the epilogues of pm_fft.h"""
    x = model_bins(audio, defect)
    magnitude = (x * x + 1e-6).sqrt()
    basis = R.mel_basis().double()
    span = spans(basis)
    if defect in ('mel_span_short_lo', 'mel_span_short_hi',
                  'mel_offset_shifted'):
        values = compacted(basis)
        rows = []
        for m, (lo, hi, offset) in enumerate(span):
            if m == 40:
                lo += defect == 'mel_span_short_lo'
                hi -= defect == 'mel_span_short_hi'
                offset += (defect == 'mel_offset_shifted') + \
                    (defect == 'mel_span_short_lo')
            row = torch.zeros(BINS, dtype=torch.float64)
            row[lo:hi] = values[offset:offset + hi - lo]
            rows.append(row)
        basis = torch.stack(rows)
    log_mel = torch.log(torch.matmul(basis, magnitude))
    raw = 10. * torch.log10((x * x).clamp_min(1e-10))
    top = raw.amax((1, 2), True)
    if defect == 'floor_of_neighbour':
        top = top.roll(1, 0)
    weights = torch.from_numpy(R.perceptual_weights())
    if defect == 'floor_after_weights':
        db = torch.maximum(raw + weights, top - TOP_DB)
    else:
        db = torch.maximum(raw, top - TOP_DB) + weights
    db = db.clamp_min(MIN_DB)
    # EPI 5: band j = bins 64 j .. 64 j + 63, bin 512 joins band 7 (/ 65)
    owner = torch.arange(BINS) // 64
    owner[512] = 7
    if defect == 'lane0_bands':
        owner[[448, 384, 320]] -= 1
    if defect == 'bin512_left_out':
        owner[512] = 8
    sums = torch.zeros(db.shape[0], 9, db.shape[2], dtype=torch.float64)
    sums.index_add_(1, owner, db)
    count = torch.tensor([64.] * 7 + [65.])[None, :, None]
    if defect in ('band7_by_64', 'bin512_left_out'):
        count[0, 7, 0] = 64.
    return {'magnitude': magnitude, 'log_mel': log_mel, 'db': db,
            'bands': {8: sums[:, :8] / count}}


def model_figures(name, defect=None):
    out = model_outputs(cases()[name].double().numpy(), defect)
    return figures(case_truth(name), out['magnitude'], out['log_mel'],
                   out['db'], out['bands'])

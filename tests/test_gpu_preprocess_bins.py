"""The LDS real-FFT kernel behind preprocess.spectrogram.from_audio and
preprocess.loudness.from_audio (pm_stft_fft_kernel, pm_fft.h), every bin of
every frame against the float64 contract of tests/preprocess_oracle.py, under
that file's fp32 error models, at K = 4 x the figure that torch's own fp32
evaluation reaches (oracle.K: magnitude 62.08, log-mel 15.28, dB per bin
15.54, band means 1.66).

Cases (oracle.cases): unit impulses in both reflections and the interior,
bin-centred cosines at the self-paired bins, lane 0's partner bins and every
64-bin band edge, the same over a noise floor that puts a quarter of the dB
bins on max - 80, silence / sub-clamp noise / a full-scale square / rows 60 dB
apart / DC + Nyquist, N from 385 to 1153 at B = 3, T from 1 to 35 at 16 and
32 frames a group, an utterance whose floor falls 5e-4 dB to either side of a
group's minimum, and the persistent walk built from the reported grid.
Structure, bit for bit: every row equals its stand-alone call, NaN guards
around the audio and behind the outputs (through the C entries, at an odd
storage offset), one-pass loudness equals two-pass, silence is MIN_DB.
Custom filterbanks go through pm_stft_mel_prepare / pm_stft_mel with their
compact tables read back.

Measured on an MI355X (printed by the tests):
largest error over its model, device (torch's fp32 on the CPU as it takes the
transform on an AVX-512 processor, same case; on the common path, which sets
the gates, the cosines give it 15.52 / 3.82 / 0.53 and the frame counts at most
3.92 / 0.99 / 3.89):
magnitude: noise 0.46 (0.59), impulses 0.58 (1.14), cosines 6.50 (2.66),
cosines over floor 2.89 (2.14), levels 1.16 (1.98), lengths at most 1.68
(1.39), frame counts at most 2.93 (2.79), walk 3.86 (4.20); log-mel, the
largest of fused, clamped and two-step: 0.34 (0.18), 0.45 (0.47), 0.68 (0.49),
1.09 (0.60), 0.49 (0.54), lengths 0.39 (0.53), frame counts 0.72 (0.91), walk
1.31 (1.30); dB per bin: 0.75 (0.68), 0.34 (0.78), 1.01 (0.53), 2.76 (1.91),
1.34 (1.25), lengths 1.67 (1.38), frame counts 2.89 (2.58), walk 3.81 (4.17);
band means, the largest over 8, 1, 2, 3, 5, 7, 16 bands: 0.66, 1.11 (one band,
impulses), 0.00, 0.07, 0.67, lengths 1.04, frame counts 0.10, walk 0.07 (the
CPU's over 8, 1 and 5 bands: at most 0.42); the 8 bands alone at most 0.18.
The frame-count cases give the same digits at 16 and 32 frames a group.
Custom filterbanks: one 0.06, edges 0.27, dense 0.05, cap 0.23, cap + 1 0.23.
The file takes 5 s.
"""
import ctypes

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.preprocess import loudness, spectrogram

import preprocess_oracle as oracle
import restatement as R
import util

pytestmark = pytest.mark.gpu

BANDS = (8, 1, 2, 3, 5, 7, 16, None)
GUARD = 33              # NaN floats around the audio: an odd storage offset
NAN = float('nan')


def rows_of(bands):
    return oracle.BINS if bands is None else bands


def magnitude(audio):
    out = spectrogram.from_audio(audio[:, None])
    return out.reshape(audio.shape[0], oracle.BINS, -1)


def log_mel(audio, threshold=None):
    out = spectrogram.from_audio(
        audio[:, None], mels=True,
        log_dynamic_range_compression_threshold=threshold)
    return out.reshape(audio.shape[0], R.NUM_MELS, -1)


def loud(audio, bands):
    out = loudness.from_audio(audio, bands)
    return out.reshape(audio.shape[0], rows_of(bands), -1)


@pytest.fixture
def group_setting():
    """set(frames) for the test; 16 frames a group and two passes afterwards"""
    lib = _lib.lib()
    try:
        yield lambda frames: _lib.check(lib.pm_stft_set_frames_per_group(frames))
    finally:
        _lib.check(lib.pm_stft_set_frames_per_group(16))
        _lib.check(lib.pm_stft_set_loudness_passes(2))


def one_pass(audio):
    """The 8-band loudness by the optimistic schedule (EPI 6, then EPI 5
    where a group's minimum lies under the floor)"""
    lib = _lib.lib()
    try:
        _lib.check(lib.pm_stft_set_loudness_passes(1))
        return loud(audio, 8)
    finally:
        _lib.check(lib.pm_stft_set_loudness_passes(2))


def guarded(audio_cpu, device):
    """The audio inside a larger NaN-filled allocation, NaN directly before
    the first and behind the last sample, its first sample at an odd offset"""
    batch, samples = audio_cpu.shape
    store = torch.full((batch * samples + 2 * GUARD,), NAN, device=device)
    view = store[GUARD:GUARD + batch * samples].view(batch, samples)
    view.copy_(audio_cpu)
    assert view.is_contiguous() and view.storage_offset() % 2 == 1
    assert store[GUARD - 1].isnan() and store[GUARD + batch * samples].isnan()
    return view


def through_c_entries(audio, prepared=None, mels=R.NUM_MELS):
    """magnitude, log-mel and every loudness shape written through the C
    entries into buffers with NaN guard floats behind the last row; returns
    the outputs after asserting that the guards are untouched"""
    lib = _lib.lib()
    batch, samples = audio.shape
    frames = samples // oracle.HOP
    device = audio.device

    def buffer(rows):
        return torch.full((batch * rows * frames + 64,), NAN, device=device)

    def taken(out, rows):
        torch.cuda.synchronize()
        assert out[batch * rows * frames:].isnan().all(), rows
        return out[:batch * rows * frames].view(batch, rows, frames)

    results = {}
    out = buffer(oracle.BINS)
    _lib.check(lib.pm_stft_magnitude(
        _lib.ptr(audio), _lib.ptr(out), batch, samples, None, 0,
        _lib.stream()))
    results['magnitude'] = taken(out, oracle.BINS)
    if prepared is None:
        prepared = spectrogram._prepared_mel_basis(device)
    out = buffer(mels)
    _lib.check(lib.pm_stft_mel(
        _lib.ptr(audio), prepared.data_ptr(), _lib.ptr(out), batch, samples,
        mels, 0, 0., _lib.stream()))
    results['log_mel'] = taken(out, mels)
    weights = loudness.perceptual_weights_tensor(device)
    size = lib.pm_loudness_scratch_bytes(batch, samples)
    scratch = torch.empty(max(size, 1), dtype=torch.uint8, device=device)
    for bands in BANDS:
        out = buffer(rows_of(bands))
        _lib.check(lib.pm_loudness(
            _lib.ptr(audio), _lib.ptr(weights), _lib.ptr(out), batch, samples,
            rows_of(bands), promonet_amd.MIN_DB, scratch.data_ptr(),
            scratch.numel(), _lib.stream()))
        results[bands] = taken(out, rows_of(bands))
    return results


def held(kind, family, got, want, bound, detail):
    """Print the figure, then hold it under K"""
    figure = oracle.figure(got, want, bound)
    print(f'{detail} {kind}: {figure:.3f} (gate {oracle.K[family]:.2f})')
    util.check(figure, oracle.K[family], f'preprocess_bins/{kind}', detail)
    return figure


def clamp_threshold(want):
    """A log-mel threshold that bites on part of the tensor"""
    finite = want[torch.isfinite(want)]
    threshold = finite.median().float().item()       # (exact in fp32)
    clamped = want.clamp_min(threshold)
    assert (clamped == threshold).any() and (clamped > threshold).any()
    return threshold, clamped


def compare_all(audio_cpu, t, device, detail, every_band=True):
    """Every output of one batch against the oracle per bin, then the
    structural checks. Returns the figures by kind."""
    assert promonet_amd.LOG_DYNAMIC_RANGE_COMPRESSION_THRESHOLD is None
    audio = audio_cpu.to(device)
    figures = {}
    got = {'magnitude': magnitude(audio), 'log_mel': log_mel(audio)}
    figures['magnitude'] = held(
        'magnitude', 'magnitude', got['magnitude'], t['magnitude'],
        oracle.magnitude_bound(t), detail)
    bound = oracle.mel_bound(t)
    figures['log_mel'] = held(
        'log_mel', 'log_mel', got['log_mel'], t['log_mel'], bound, detail)
    two_step = spectrogram.linear_to_mel(got['magnitude'])
    figures['two_step'] = held(
        'log_mel_two_step', 'log_mel', two_step, t['log_mel'], bound, detail)
    threshold, clamped = clamp_threshold(t['log_mel'])
    figures['clamped'] = held(
        'log_mel_clamped', 'log_mel', log_mel(audio, threshold), clamped,
        bound, detail)
    for bands in BANDS if every_band else (8, None):
        got[bands] = loud(audio, bands)
        if bands is None:
            figures['db_bin'] = held(
                'db_bin', 'db_bin', got[None], t['db'], oracle.db_bound(t),
                detail)
        else:
            figures[f'bands_{bands}'] = held(
                f'bands_{bands}', 'band_mean', got[bands],
                R.band_average(t['db'], bands), oracle.band_bound(t, bands),
                detail)
    # one pass writes the bits of two
    assert torch.equal(one_pass(audio), got[8]), detail
    return audio, got, figures


CASES = list(oracle.cases())
SETTINGS = [(name, 16) for name in CASES] + \
    [(name, 32) for name in CASES if name.startswith('frames_')]


@pytest.mark.parametrize('name,frames_per_group', SETTINGS)
def test_case_per_bin(device, group_setting, name, frames_per_group):
    """Every case of the oracle's table: per bin under K x the fp32 model,
    each row equal to its stand-alone call, the NaN guards around the audio
    and behind the outputs, one pass equal to two"""
    group_setting(frames_per_group)
    audio_cpu, t = oracle.cases()[name], oracle.case_truth(name)
    batch, samples = audio_cpu.shape
    detail = f'{name}/{frames_per_group}'
    if name == 'cosines_floor' or name.startswith('frames_'):
        under, over = oracle.floor_shares(t)
        assert under >= .2 and over >= .2, (name, under, over)
    audio, got, _ = compare_all(audio_cpu, t, device, detail)
    # each row alone: the same bits
    if batch > 1:
        for row in range(batch):
            alone = audio[row:row + 1].clone()
            assert torch.equal(magnitude(alone)[0], got['magnitude'][row])
            assert torch.equal(log_mel(alone)[0], got['log_mel'][row])
            for bands in (8, 3, None):
                assert torch.equal(loud(alone, bands)[0], got[bands][row])
    # NaN all around the audio, its first sample at an odd offset; outputs
    # through the C entries with NaN behind them
    results = through_c_entries(guarded(audio_cpu, device))
    for key, value in results.items():
        assert not value.isnan().any(), (detail, key)
        assert torch.equal(value, got[key]), (detail, key)


def test_silence_is_min_db(device):
    audio = torch.zeros(2, 5 * 256 + 3, device=device)
    for bands in BANDS:
        assert (loud(audio, bands) == promonet_amd.MIN_DB).all()
    assert (one_pass(audio) == promonet_amd.MIN_DB).all()
    # (and the silent row of `levels` beside its loud neighbours)
    levels = oracle.cases()['levels'].to(device)
    for bands in BANDS:
        assert (loud(levels, bands)[0] == promonet_amd.MIN_DB).all()
    assert (one_pass(levels)[0] == promonet_amd.MIN_DB).all()
    want = torch.full((), 1e-6, dtype=torch.float64).sqrt()
    assert (magnitude(audio).double().cpu() - want).abs().max() <= \
        2. ** -22 * want


@pytest.mark.parametrize('side', [+1, -1])
def test_floor_decision_of_the_optimistic_pass(device, side):
    """The first 16-frame group is silent (every bin on the 1e-10 clamp:
    -100 dB) and the utterance's floor lies 5e-4 dB above (+1: the group is
    transformed again) or below (-1: it is skipped) - asserted from the
    oracle; one pass gives the bits of two on both sides"""
    name = 'floor_above' if side > 0 else 'floor_below'
    audio_cpu, t = oracle.cases()[name], oracle.case_truth(name)
    minimum = t['raw_db'][0, :, :16].min().item()
    floor = t['floor'].item()
    assert abs(minimum + 100.) < 1e-9 and 0 < side * (floor - minimum) < 1e-3
    audio = audio_cpu.to(device)
    two = loud(audio, 8)
    assert torch.equal(one_pass(audio), two)
    held('bands_8', 'band_mean', two, R.band_average(t['db'], 8),
         oracle.band_bound(t, 8), name)
    # the floor does what the side says to the silent group: under it the
    # bins are lifted to the floor, 5e-4 dB above MIN_DB + weight
    per_bin = loud(audio, None)[0, :, :16].double().cpu()
    weights = torch.from_numpy(R.perceptual_weights())
    want = (max(floor, -100.) + weights).clamp_min(promonet_amd.MIN_DB)
    assert (per_bin - want).abs().max() < 1e-4


def geometry(transform, batch, samples):
    total, grid = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().pm_stft_launch_info(
        transform, batch, samples, ctypes.byref(total), ctypes.byref(grid)))
    return total.value, grid.value


def test_persistent_walk_per_bin(device, group_setting):
    """The smallest batch whose groups exceed the resident workgroups of
    every transform (magnitude 1, log-mel 4, loudness 2 / 5, 6 / 5 and the
    generic 2 / 3), by a handful, built from the reported grid; cosines over
    their floors at five levels, held per bin"""
    group_setting(16)
    # (a batch far past any grid reports what the device holds at once)
    grids = {transform: geometry(transform, 4096, 400 * 256)[1]
             for transform in (1, 2, 3, 4, 5, 6)}
    audio_cpu, groups = oracle.walk_case(max(grids.values()))
    batch, samples = audio_cpu.shape
    assert groups % 8 != 0 and audio_cpu.numel() * 4 < 32 << 20
    for transform, resident in grids.items():
        total, grid = geometry(transform, batch, samples)
        assert total == batch * groups and grid == resident
        assert total > grid and grid % 8 == 0, (transform, total, grid)
    assert batch * groups - max(grids.values()) < 16
    t = oracle.truth(audio_cpu)
    under, over = oracle.floor_shares(t)
    assert under >= .2 and over >= .2
    audio, got, _ = compare_all(audio_cpu, t, device, 'walk', every_band=False)
    alone = audio[3:4].clone()
    assert torch.equal(magnitude(alone)[0], got['magnitude'][3])
    assert torch.equal(log_mel(alone)[0], got['log_mel'][3])
    assert torch.equal(loud(alone, 8)[0], got[8][3])


###############################################################################
# Custom filterbanks: pm_mel_csr_kernel and both filter paths of EPI 4
###############################################################################


def triangle(lo, peak, hi, height=1.):
    row = torch.zeros(oracle.BINS)
    for f in range(lo, hi):
        row[f] = height * (
            (f - lo + 1) / (peak - lo + 1) if f <= peak else
            (hi - f) / (hi - peak))
    return row


def dense_rows(lengths, seed):
    """Rows of one dense span each, at staggered starts"""
    generator = torch.Generator().manual_seed(seed)
    basis = torch.zeros(len(lengths), oracle.BINS)
    for m, length in enumerate(lengths):
        lo = (m * 37) % (oracle.BINS - length + 1)
        basis[m, lo:lo + length] = torch.rand(length, generator=generator) + .1
    return basis


def filterbanks():
    interior = triangle(100, 120, 160)
    interior[110:115] = 0.
    interior[130] = 0.
    return {
        'one': triangle(200, 230, 300)[None],
        'edges': torch.stack([
            triangle(0, 4, 12), torch.zeros(oracle.BINS), interior,
            triangle(490, 505, 513), triangle(3, 3, 4)]),
        'dense': torch.rand(
            6, oracle.BINS, generator=torch.Generator().manual_seed(9)) + .01,
        'cap': dense_rows([26] * 48 + [25] * 32, 10),
        'cap_plus_one': dense_rows([27] + [26] * 47 + [25] * 32, 11),
    }


COUNTS = {'one': 100, 'edges': 12 + 0 + 60 + 23 + 1, 'dense': 3078,
          'cap': 2048, 'cap_plus_one': 2049}


@pytest.mark.parametrize('name', list(COUNTS))
def test_custom_filterbank(device, name):
    """M = 1, an all-zero row (-inf, or the threshold), interior zeros, spans
    touching bins 0 and 512, a one-bin span, M no multiple of 4; the dense
    bank and the one a value over PM_FFT_MEL_CAP run the global-memory loop.
    The prepared table and the compacted values are read back."""
    lib = _lib.lib()
    basis = filterbanks()[name]
    mels = basis.shape[0]
    span = oracle.spans(basis)
    count = span[-1][2] + span[-1][1] - span[-1][0]
    assert count == COUNTS[name]
    size = lib.pm_stft_mel_scratch_bytes(mels)
    prepared = torch.zeros(size, dtype=torch.uint8, device=device)
    on_device = basis.to(device).contiguous()
    _lib.check(lib.pm_stft_mel_prepare(
        _lib.ptr(on_device), mels, prepared.data_ptr(), prepared.numel(),
        _lib.stream()))
    torch.cuda.synchronize()
    table = prepared[:4 * (3 * mels + 1)].view(torch.int32).cpu()
    assert table[:3 * mels].view(mels, 3).tolist() == [list(s) for s in span]
    assert table[3 * mels].item() == count
    assert (count > 2048) == (name in ('dense', 'cap_plus_one'))
    start = (4 * (3 * mels + 1) + 255) // 256 * 256
    values = prepared[start:start + 4 * count].view(torch.float32).cpu()
    assert torch.equal(values, oracle.compacted(basis))

    audio_cpu = oracle.cases()['cosines_floor']
    t = oracle.case_truth('cosines_floor')
    audio = audio_cpu.to(device)
    batch, samples = audio.shape
    want = torch.log(torch.matmul(basis.double(), t['magnitude']))
    bound = oracle.mel_bound(t, basis, want)
    empty = [m for m, (lo, hi, _) in enumerate(span) if hi == lo]
    assert (name == 'edges') == bool(empty)
    got = through_c_entries(audio, prepared, mels)['log_mel']
    held(f'filterbank_{name}', 'log_mel', got, want, bound, name)
    for m in empty:
        assert (got[:, m] == float('-inf')).all()
    # clamped: the empty row gives the threshold
    threshold, clamped = clamp_threshold(want)
    out = torch.empty(batch, mels, samples // 256, device=device)
    _lib.check(lib.pm_stft_mel(
        _lib.ptr(audio), prepared.data_ptr(), _lib.ptr(out), batch, samples,
        mels, 1, threshold, _lib.stream()))
    held(f'filterbank_{name}_clamped', 'log_mel', out, clamped, bound, name)
    for m in empty:
        assert (out[:, m] == torch.tensor(threshold).float()).all()
    # the two-step path on the same bank
    two_step = torch.empty_like(out)
    spec = magnitude(audio)
    _lib.check(lib.pm_linear_to_mel(
        _lib.ptr(spec), _lib.ptr(on_device), _lib.ptr(two_step), batch,
        oracle.BINS, mels, samples // 256, 0, 0., _lib.stream()))
    held(f'filterbank_{name}_two_step', 'log_mel', two_step, want, bound, name)


###############################################################################
# Non-finite audio
###############################################################################


def test_nan_sample_poisons_exactly_the_frames_that_see_it(device):
    """A NaN sample makes the magnitude and log-mel frames whose window sees
    it NaN in every row, and no other: the frames from 4 before to 4 after
    keep the bits of the clean run. (Loudness with non-finite audio is out of
    scope: the kernel's fmaxf clamps drop NaN where the reference's
    np.maximum propagates it to the whole utterance.)"""
    clean = oracle.noise(2, 40 * 256 + 77, 21)
    for position in (0, 300, 20 * 256 + 1, 40 * 256 + 76):
        audio = clean.clone()
        audio[1, position] = NAN
        # frame t sees padded positions [256 t, 256 t + 1024): the sample
        # itself at position + 384 and its reflections
        samples = audio.shape[1]
        copies = {position + 384}
        if 0 < position <= 384:
            copies.add(384 - position)
        if samples - 1 - 384 <= position < samples - 1:
            copies.add(384 + 2 * (samples - 1) - position)
        frames = samples // 256
        seen = torch.tensor([
            any(256 * f <= c < 256 * f + 1024 for c in copies)
            for f in range(frames)])
        assert 1 <= seen.sum() <= 6
        first = int(seen.nonzero()[0])
        last = int(seen.nonzero()[-1])
        near = torch.zeros(frames, dtype=torch.bool)
        near[max(first - 4, 0):last + 5] = True
        near &= ~seen
        assert near.any()
        for function in (magnitude, log_mel):
            want = function(clean.to(device)).cpu()
            got = function(audio.to(device)).cpu()
            assert torch.equal(got[0], want[0])
            assert got[1][:, seen].isnan().all(), (function, position)
            assert torch.equal(got[1][:, ~seen], want[1][:, ~seen])
            assert torch.equal(got[1][:, near], want[1][:, near])

"""The interpolated-sinc resampler and data augmentation on the host: the
oracle's three evaluations held to each other and to the product's host path,
the table, planted defects, the argument checks of pm_resample_interp and the
file flow of promonet_amd.data.augment. No GPU.

Error bound used here and in test_gpu_augment.py (derived, not measured). An
output is sum_k w_k x_k over K = taps products, w_k = win_k + eta_k delta_k.
With u = 2^-24, to first order in u:
  - win_k, delta_k and eta_k are each rounded to fp32 and the weight's fma
    rounds once more, so the fp32 weight is within
    u (|win_k| + 2 |eta_k delta_k| + |w_k|) <= u (2 |w_k| + 3 |eta_k delta_k|)
    of w_k (|win_k| <= |w_k| + |eta_k delta_k|);
  - K fmas in one chain add at most K u sum_k |w_k| |x_k|.
delta is the table's slope over 1 / 512 of a zero crossing, so
sum_k |eta_k delta_k| |x_k| <= sum_k |w_k| |x_k| wherever a wing holds more
than a handful of samples; `slope_holds` asserts it for the inputs used, from
the float64 evaluation alone. Then
  |y - y64| <= (K + 5) u sum_k |w_k| |x_k|.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd import _lib, resampy

import resampy_oracle as oracle

BOUND_C = 5
U = 2. ** -24


def slope_holds(scale, slope):
    return (slope <= scale).all()


# ---------------------------------------------------------------------------
# The table
# ---------------------------------------------------------------------------
def test_table_properties():
    win, delta = oracle.tables64()
    assert win.shape == delta.shape == (32769,) == (resampy.TABLE,)
    assert win[0] == oracle.ROLLOFF and delta[-1] == 0
    assert (delta[:-1] == win[1:] - win[:-1]).all()
    # sinc(rolloff j / P) changes sign at every multiple of P / rolloff
    crossings = 0
    k = 1
    while k * oracle.P / oracle.ROLLOFF < oracle.N:
        at = k * oracle.P / oracle.ROLLOFF
        below, above = int(np.floor(at)), int(np.ceil(at))
        assert win[below] * win[above] < 0, k
        crossings += 1
        k += 1
    assert crossings == 60
    signs = np.sign(win[:-1])
    assert (signs[1:] != signs[:-1]).sum() == crossings
    # downsampling scales the table in float64, before the differences
    scaled, scaled_delta = oracle.tables64(48000, 22050)
    assert (scaled == win * (22050 / 48000)).all()
    assert (scaled_delta[:-1] == scaled[1:] - scaled[:-1]).all()
    assert (oracle.tables64(22050, 48000)[0] == win).all()
    # the product's tables: numpy's kaiser against the I0 written out here
    for pair in [(1, 1), (48000, 22050), (22050, 44100)]:
        mine, mine_delta = resampy.tables(*pair)
        want, want_delta = oracle.tables32(*pair)
        assert mine.dtype == mine_delta.dtype == np.float32
        assert np.abs(mine.astype(np.float64) - want).max() <= 2. ** -24
        assert (mine_delta[-1] == 0) and mine.shape == (32769,)
        assert np.abs(mine_delta.astype(np.float64) - want_delta).max() < 1e-9


def test_tile_and_the_ratios_it_refuses():
    library = _lib.lib()
    for orig, new in oracle.PAIRS + oracle.INTEGER_PAIRS + [
            (5, 1), (1, 4), (53, 10), (1, 1000), (22050, 22050),
            (int(.5 * 44100), 44100), (int(2. * 44100), 44100),
            (int(1.2345 * 44100), 44100), (96000, 22050),
            (2 ** 21 - 1, 2 ** 20)]:
        assert library.pm_resample_interp_tile(orig, new) == oracle.TILE
        assert resampy.tile(orig, new) == oracle.TILE
        # the segment the oracle's geometry predicts fits the LDS
        span = ((oracle.TILE - 1) * orig + new - 1) // new + 1
        assert span + 2 * oracle.wing_of(orig, new) <= oracle.LDS_FLOATS
    assert int(1.2345 * 44100) == 54441
    # 48 k -> 22.05 k: 139 taps either side
    assert oracle.step_of(48000, 22050) == 235
    assert oracle.wing_of(48000, 22050) == 139
    for orig, new, message in [
            (0, 1, 'at least 1'), (1, 0, 'at least 1'), (-3, 2, 'at least 1'),
            (2 ** 21, 1, 'below'), (1, 2 ** 21, 'below'),
            (7, 1, 'LDS'), (8, 1, 'LDS'), (48000, 50, 'LDS'), (1000, 1, 'LDS')]:
        assert library.pm_resample_interp_tile(orig, new) == _lib.PM_EINVAL
        assert message in library.pm_last_error().decode(), (orig, new)
    with pytest.raises(_lib.LibraryError, match='LDS'):
        resampy.resample(torch.zeros(1, 64), 8, 1)
    with pytest.raises(ValueError, match='kaiser_best'):
        resampy.resample(torch.zeros(1, 64), 2, 1, filter='kaiser_fast')


def call(library, **overrides):
    """pm_resample_interp with valid sizes and fake, never dereferenced,
    pointers"""
    a = dict(x=0x1000, lengths=None, orig=0x2000, new=0x3000, win=0x4000,
             delta=0x5000, out=0x6000, rows=2, n_in=1000, x_stride=1000,
             n_out=460, out_stride=460)
    a.update(overrides)
    return library.pm_resample_interp(
        a['x'], a['lengths'], a['orig'], a['new'], a['win'], a['delta'],
        a['out'], a['rows'], a['n_in'], a['x_stride'], a['n_out'],
        a['out_stride'], None)


def test_signature_and_argument_checks():
    restype, argtypes = _lib.SIGNATURES['pm_resample_interp']
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert _lib.SIGNATURES['pm_resample_interp_tile'] == (
        ctypes.c_int, [ctypes.c_int, ctypes.c_int])
    library = _lib.lib()
    for overrides, message in [
            (dict(rows=-1), 'negative'), (dict(n_in=-1), 'negative'),
            (dict(n_out=-1), 'negative'),
            (dict(x=None), 'null'), (dict(orig=None), 'null'),
            (dict(new=None), 'null'), (dict(win=None), 'null'),
            (dict(delta=None), 'null'), (dict(out=None), 'null'),
            (dict(x_stride=999), 'stride'), (dict(out_stride=459), 'stride'),
            (dict(rows=2 ** 31 - 1, n_out=2048, out_stride=2048),
             'workgroups')]:
        code = call(library, **overrides)
        assert code == _lib.PM_EINVAL, overrides
        assert message in library.pm_last_error().decode(), overrides
        with pytest.raises(_lib.LibraryError):
            _lib.check(code)
    # nothing to do is not an error, and launches nothing
    assert call(library, rows=0) == 0
    assert call(library, n_out=0, out_stride=0) == 0


# ---------------------------------------------------------------------------
# The three evaluations
# ---------------------------------------------------------------------------
def three_lengths(orig, new):
    """The longest wing + 1, one tile's inputs + 1 and the third-tile length"""
    lengths = oracle.lengths_of(orig, new)
    return [lengths[-4], lengths[-2], lengths[-1]]


MEASURED_POSITION_DIFFERENCE = 7.4e-13


@pytest.mark.parametrize('orig,new', oracle.PAIRS)
def test_integer_against_float_positions(orig, new):
    """resampy's float64 positions against the contract's integers, on the
    six rate pairs at 3 lengths each. Measured here (offsets that differ of
    all offsets, largest |difference| of the outputs, inputs at peak 1):

        48 000 -> 22 050    720 of 7 300   7.3e-13
        54 441 -> 44 100      0 of 7 304   5.0e-13
        22 050 -> 44 100      0 of 7 444   4.4e-16
        22 051 -> 22 050      0 of 7 306   4.9e-13
        24 000 -> 48 000      0 of 7 444   4.4e-16
        96 000 -> 48 000      0 of 7 298   2.2e-16

    At 48 000 -> 22 050 rem P / D is an integer for every fifth rem, and the
    float64 product lands just under it: the offset is one lower and eta just
    under 1. The table is continuous in the phase, so the value moves by
    rounding error only. The differences themselves come from time - n, which
    loses the bits of n. The gate is 10 times the largest figure. This guards
    the integer form against the published loop, not the kernel."""
    differ = total = 0
    worst = 0.
    for length in three_lengths(orig, new):
        x = oracle.signal(length)
        literal, offsets = oracle.literal64(x, orig, new)
        y, scale, slope, taps, mine = oracle.contract64(x, orig, new)
        assert literal.shape == y.shape == (length * new // orig,)
        differ += int((offsets != mine).sum())
        total += offsets.size
        worst = max(worst, np.abs(literal - y).max())
    print(f'{orig} -> {new}: {differ} of {total} offsets differ, '
          f'largest difference {worst:.3e}')
    assert worst <= 10 * MEASURED_POSITION_DIFFERENCE


@pytest.mark.parametrize('orig,new', oracle.PAIRS)
def test_fp32_chain_within_the_bound_of_float64(orig, new):
    win, delta = oracle.tables32(orig, new)
    worst = 0.
    most_taps = 0
    for length in oracle.lengths_of(orig, new):
        x = oracle.signal(length)
        want, scale, slope, taps, _ = oracle.contract64(x, orig, new)
        got = oracle.chain32(x, orig, new, win, delta)
        if length > 2:
            assert slope_holds(scale, slope), length
        bound = (taps + BOUND_C) * U * scale
        error = np.abs(got.astype(np.float64) - want)
        assert (error <= bound).all(), (length, (error / bound).max())
        if error.size:
            worst = max(worst, (error / np.maximum(bound, 1e-300)).max())
            most_taps = max(most_taps, int(taps.max()))
    print(f'{orig} -> {new}: worst error / bound {worst:.3f}, '
          f'up to {most_taps} taps')
    # rem = 0: the left wing is whole, the right one starts a step in
    assert most_taps == 2 * oracle.wing_of(orig, new) - 1


def test_descending_order_changes_bits():
    """torch.equal to chain32 pins the order of the chain: summing a wing
    from its last tap to its first gives other bits"""
    for orig, new in oracle.PAIRS:
        length = oracle.lengths_of(orig, new)[3]
        x = oracle.signal(length)
        win, delta = oracle.tables32(orig, new)
        ascending = oracle.chain32(x, orig, new, win, delta)
        descending = oracle.chain32(x, orig, new, win, delta, descending=True)
        assert (ascending != descending).any(), (orig, new)
        assert np.abs(ascending - descending).max() < 1e-5


@pytest.mark.parametrize('orig,new', oracle.PAIRS)
def test_host_path_is_the_chain(orig, new):
    """promonet_amd.resampy's host path and the oracle's chain32 were written
    apart; they must agree bit for bit, ragged rows and zero tails included"""
    lengths = oracle.lengths_of(orig, new)[:4] + [0]
    n_in = max(lengths)
    x = np.stack([oracle.signal(n_in, seed) for seed in range(len(lengths))])
    got, out_lengths = resampy.resample(
        torch.from_numpy(x), orig, new, lengths=lengths)
    n_out = n_in * new // orig
    assert got.shape == (len(lengths), n_out) and got.dtype == torch.float32
    assert out_lengths == [length * new // orig for length in lengths]
    win, delta = oracle.tables32(orig, new)
    mine, mine_delta = resampy.tables(orig, new)
    for row, length in enumerate(lengths):
        want = oracle.chain32(x[row], orig, new, mine, mine_delta, length,
                              n_out)
        assert np.array_equal(got[row].numpy(), want), (row, length)
    # the two table builds differ by an ulp in places at most
    assert np.abs(mine.astype(np.float64) - win).max() <= U
    # one row, int rates, no lengths: a plain tensor comes back
    assert lengths[3] == n_in
    alone = resampy.resample(torch.from_numpy(x[3]), orig, new)
    assert torch.equal(alone, got[3])
    # a float64 tensor and a transposed view give the same bits
    whole = resampy.resample(torch.from_numpy(x[:2]), orig, new)
    view = torch.from_numpy(x[:2]).double().T.contiguous().T
    assert not view.is_contiguous()
    assert torch.equal(resampy.resample(view, orig, new), whole)


def test_host_path_mixes_rates():
    pairs = oracle.PAIRS
    n_in = 300
    x = torch.from_numpy(np.stack(
        [oracle.signal(n_in, seed) for seed in range(len(pairs))]))
    lengths = [300, 299, 150, 0, 1, 257]
    got, out_lengths = resampy.resample(
        x, [pair[0] for pair in pairs], [pair[1] for pair in pairs],
        lengths=lengths)
    assert got.shape == (6, 600)
    for row, (orig, new) in enumerate(pairs):
        want = resampy.resample(x[row, :lengths[row]], orig, new)
        assert out_lengths[row] == want.shape[0]
        assert torch.equal(got[row, :want.shape[0]], want)
        assert not got[row, want.shape[0]:].any()
    with pytest.raises(ValueError, match='rows'):
        resampy.resample(x, [1, 2], 3)


# ---------------------------------------------------------------------------
# Planted defects
# ---------------------------------------------------------------------------
def integer_lengths(orig, new):
    lengths = oracle.lengths_of(orig, new)
    return [lengths[0], lengths[3], lengths[-2], lengths[-1]]


@pytest.mark.parametrize('orig,new', oracle.INTEGER_PAIRS)
def test_planted_defects_change_outputs(orig, new):
    """Every defect must show at the shapes the device test runs"""
    changed = {defect: False for defect in oracle.DEFECTS}
    other_rates = False
    for n_in in integer_lengths(orig, new):
        x, win, delta = oracle.integer_case(orig, new, 3, n_in)
        n_out = n_in * new // orig + 5
        good = oracle.integer_outputs(x[0], win, delta, orig, new, n_in,
                                      n_out)
        assert not np.isnan(good).any()
        assert not good[n_in * new // orig:].any()
        for defect in oracle.DEFECTS:
            bad = oracle.integer_outputs(x[0], win, delta, orig, new, n_in,
                                         n_out, defect)
            same = (bad == good) | (np.isnan(bad) & np.isnan(good))
            changed[defect] |= not same.all()
        # a row using another row's rates
        swapped = oracle.integer_outputs(
            x[0], win, delta, new, orig, n_in, max(n_out, n_in * orig // new))
        other_rates |= not np.array_equal(swapped[:n_out], good)
    if new >= orig:
        assert not changed.pop('step taken as P when downsampling')
    if max(orig, new) <= oracle.P:      # eta is always 0 there
        assert not changed.pop('eta and eta\' swapped')
    if n_in * new % orig == 0 and new % orig == 0:
        assert not changed.pop('last partial output written')
    assert all(changed.values()), [d for d, c in changed.items() if not c]
    assert other_rates


# ---------------------------------------------------------------------------
# Augmentation
# ---------------------------------------------------------------------------
def test_sample_is_the_formula():
    torch.manual_seed(7)
    got = promonet_amd.data.augment.sample(4096)
    torch.manual_seed(7)
    uniform = torch.rand(4096)
    low, high = torch.log2(torch.tensor(.5)), torch.log2(torch.tensor(2.))
    want = 2 ** (low + uniform * (high - low))
    bumped = (want * 100).to(torch.int) == 100
    assert bumped.sum() > 0
    want[bumped] += 1
    assert torch.equal(got, want)
    assert ((got >= .5) & (got <= 3.)).all()
    assert not ((got * 100).to(torch.int) == 100).any()
    assert (got[bumped] >= 2.).all()


def write_wav(file, rate, samples, seed, channels=1):
    rng = np.random.default_rng(seed)
    data = (rng.uniform(-.4, .4, size=(samples, channels)) * 32768)
    import scipy.io.wavfile
    scipy.io.wavfile.write(file, rate, data.astype(np.int16).squeeze())


def test_files_names_and_json(tmp_path, monkeypatch):
    """augment.from_files_to_files on the host path: two short files, the
    reference's names and JSON, and the bytes of the one-file loop"""
    monkeypatch.setattr(promonet_amd, 'AUGMENT_DIR', tmp_path / 'augment')
    speaker = tmp_path / 'cache' / '0003'
    speaker.mkdir(parents=True)
    files = [speaker / '000000-100.wav', speaker / '000001-100.wav']
    write_wav(files[0], 16000, 90, 0)
    write_wav(files[1], 24000, 70, 1, channels=2)
    augment = promonet_amd.data.augment
    augment.from_files_to_files(files, 'tiny')

    torch.manual_seed(promonet_amd.RANDOM_SEED)
    pitch, loudness = augment.sample(2), augment.sample(2)
    for kind, ratios in (('pitch', pitch), ('loudness', loudness)):
        with open(tmp_path / 'augment' / f'tiny-{kind}.json') as file:
            saved = json.load(file)
        assert saved == {
            f'0003/00000{i}': f'{int(ratio * 100):03d}'
            for i, ratio in enumerate(ratios)}
        for i, ratio in enumerate(ratios):
            written = speaker / (
                f'00000{i}-{kind[0]}{int(ratio * 100):03d}.wav')
            assert written.exists(), written
            rate, audio = promonet_amd.load.decode(written)
            assert rate == promonet_amd.SAMPLE_RATE
            assert audio.shape[0] == i + 1 and audio.dtype == torch.float32
            # the one-file loop writes the same bytes
            again = tmp_path / f'{kind}{i}.wav'
            module = getattr(augment, kind)
            module.from_file_to_file(files[i], again, ratio)
            assert again.read_bytes() == written.read_bytes()
    # pitch: two passes, lengths in integers
    rate, audio = promonet_amd.load.decode(
        speaker / f'000000-p{int(pitch[0] * 100):03d}.wav')
    first = 90 * 16000 // int(pitch[0] * 16000)
    assert audio.shape[1] == first * 22050 // 16000


def test_loudness_redraws_on_the_host():
    """peak 0.9 and ratio 2 clip: the ratio is drawn again, from the global
    generator, until the shifted audio stays inside +-1"""
    audio = torch.from_numpy(oracle.signal(64))[None] * .9
    loudness = promonet_amd.data.augment.loudness
    torch.manual_seed(3)
    got, ratio = loudness.from_audio(audio, 44100, torch.tensor(2.))
    torch.manual_seed(3)
    draws = 0
    want_ratio = torch.tensor(2.)
    while (audio * float(want_ratio)).abs().max() >= 1.:
        want_ratio = promonet_amd.data.augment.sample(1)[0]
        draws += 1
    assert draws >= 1 and ratio == want_ratio and ratio * .9 < 1.
    assert got.shape == (1, 32)
    # a ratio that does not clip comes back as it is
    got, ratio = loudness.from_audio(audio, 44100, .75)
    assert ratio == .75
    want = resampy.resample(audio * float(np.float64(.75)), 44100, 22050)
    assert torch.allclose(got, want, rtol=1e-6, atol=0)

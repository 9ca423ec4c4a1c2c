"""The 'lpc' features of promonet_amd.preprocess.harmonics (pm_harmonics_lpc)
against the CPU restatement of tests/lpc_oracle.py.

Gated cases are 2048 samples (8 frames) of noise-driven signals. The target
is the float64 evaluation of Burg's recursion; the gate is 4 x the distance
of the literal float32 recursion (the reference's arithmetic) from it on the
same case, computed by tests/test_cpu_lpc.py::test_yardstick and written
here. Everything structural is exact: silence, scaling by a power of two,
ragged rows against their stand-alone calls, a replayed graph, and the
decoders on the device's own features.

Measured on an MI355X, features / coefficients error
over the float32 recursion's own (gate 4): white 1.09 / 0.80; three
resonances 0.51 / 0.014; two wide resonances 0.30 / 0.024; four resonances
0.12 / 0.004; orders 1, 2, 23: 0.94 / 0.97, 0.27 / 0.083, 0.53 / 0.015.
"""
import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd.preprocess import harmonics

import harmonics_oracle
import lpc_oracle as oracle
import util

pytestmark = pytest.mark.gpu

# (features, coefficients): float32 recursion against float64, per case
YARDSTICK = {
    'white': (5.35e-8, 3.89e-8),
    'three resonances, 40 dB floor': (2.73e-5, 3.04e-5),
    'two wide resonances': (1.30e-4, 1.75e-4),
    'four resonances, 40 dB floor': (1.30e-4, 9.66e-5),
}
RESONANT = 'three resonances, 40 dB floor'


def same(a, b):
    """Bit-for-bit equality that lets NaN equal NaN"""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(), b.nan_to_num())


@pytest.fixture(scope='module')
def signals():
    return {name: oracle.case(name) for name in oracle.CASES}


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_features_and_coefficients(device, signals, name):
    audio = signals[name]
    want, want_coefficients = oracle.features(audio)
    frames, frequencies, coefficients = harmonics.lpc_coefficients(
        torch.from_numpy(audio)[None].to(device), return_coefficients=True)
    assert frames.shape == (8, 512) and frames.dtype == torch.float32
    assert coefficients.shape == (8, 25)
    assert torch.equal(frequencies.cpu(), oracle.frequencies())
    assert (coefficients[:, 0] == 1).all()
    error = np.abs(frames.cpu().numpy().astype(np.float64) - want).max()
    coefficient_error = np.abs(
        coefficients.cpu().numpy().astype(np.float64) -
        want_coefficients).max()
    gate, coefficient_gate = YARDSTICK[name]
    print(f'{name}: features {error:.3e} ({error / gate:.3f} x the float32 '
          f'recursion), coefficients {coefficient_error:.3e} '
          f'({coefficient_error / coefficient_gate:.3f} x)')
    util.check(error, 4 * gate, f'lpc features, {name}')
    util.check(coefficient_error, 4 * coefficient_gate,
               f'lpc coefficients, {name}')


@pytest.mark.parametrize('order', [1, 2, 23])
def test_order_edges(device, signals, order):
    """The raw launch at the ends of the unrolled shift and of the
    coefficient update; the gate is 4 x the float32 recursion's own error at
    that order, computed here"""
    audio = signals[RESONANT]
    want, want_coefficients = oracle.features(audio, order=order)
    single, single_coefficients = oracle.features(
        audio, np.float32, order=order)
    frames, coefficients = harmonics.lpc(
        torch.from_numpy(audio)[None].to(device), order=order,
        return_coefficients=True)
    assert frames.shape == (1, 8, 512)
    assert coefficients.shape == (1, 8, order + 1)
    error = np.abs(frames[0].cpu().numpy().astype(np.float64) - want).max()
    coefficient_error = np.abs(
        coefficients[0].cpu().numpy().astype(np.float64) -
        want_coefficients).max()
    gate = np.abs(single - want).max()
    coefficient_gate = np.abs(single_coefficients - want_coefficients).max()
    print(f'order {order}: features {error:.3e} ({error / gate:.3f} x), '
          f'coefficients {coefficient_error:.3e} '
          f'({coefficient_error / coefficient_gate:.3f} x)')
    util.check(error, 4 * gate, f'lpc features, order {order}')
    util.check(coefficient_error, 4 * coefficient_gate,
               f'lpc coefficients, order {order}')
    with pytest.raises(promonet_amd._lib.LibraryError, match='1 to 32'):
        harmonics.lpc(torch.zeros(1, 2048, device=device), order=33)


def test_silence_and_zero_frames_are_exactly_zero(device, signals):
    frames, _, coefficients = harmonics.lpc_coefficients(
        torch.zeros(1, 2048, device=device), return_coefficients=True)
    assert frames.shape == (8, 512)
    assert torch.equal(frames, torch.zeros_like(frames))
    assert not torch.signbit(frames).any()
    assert (coefficients[:, 0] == 1).all() and (coefficients[:, 1:] == 0).all()
    # frame t is samples [256 t - 384, 256 t + 640): a burst in [3000, 4000)
    # reaches frames 10 to 17 only
    audio = torch.zeros(1, 8192)
    audio[0, 3000:4000] = torch.from_numpy(signals[RESONANT][:1000])
    frames, _ = harmonics.lpc_coefficients(audio.to(device))
    assert frames.shape == (32, 512)
    touched = [t for t in range(32)
               if 256 * t - 384 < 4000 and 256 * t + 640 > 3000]
    assert touched == list(range(10, 18))
    for t in range(32):
        if t in touched:
            assert frames[t].abs().max() > .1
        else:
            assert torch.equal(frames[t], torch.zeros(512, device=device))


def test_a_power_of_two_scale_changes_no_bit(device, signals):
    audio = torch.from_numpy(signals[RESONANT])[None].to(device)
    frames, _, coefficients = harmonics.lpc_coefficients(
        audio, return_coefficients=True)
    scaled, _, scaled_coefficients = harmonics.lpc_coefficients(
        audio * 2. ** -3, return_coefficients=True)
    assert torch.equal(scaled, frames)
    assert torch.equal(scaled_coefficients, coefficients)


LENGTHS = [255, 256, 1100, 2560]


@pytest.fixture(scope='module')
def ragged(signals):
    batch = torch.full((4, 2560), 7.)               # never read past a length
    for row, (name, length) in enumerate(zip(oracle.CASES, LENGTHS)):
        signal = np.concatenate([signals[name], signals[name][:512]])
        batch[row, :length] = torch.from_numpy(signal[:length])
    return batch


def test_each_ragged_row_equals_its_stand_alone_call(device, ragged):
    batch = ragged.to(device)
    frames, frequencies, coefficients = harmonics.lpc_coefficients(
        batch, lengths=LENGTHS, return_coefficients=True)
    assert frames.shape == (4, 10, 512) and coefficients.shape == (4, 10, 25)
    counts = [oracle.frame_count(length) for length in LENGTHS]
    assert counts == [0, 1, 4, 10]
    for row, (length, count) in enumerate(zip(LENGTHS, counts)):
        alone, _, alone_coefficients = harmonics.lpc_coefficients(
            batch[row:row + 1, :length], return_coefficients=True)
        assert alone.shape == (count, 512)
        assert torch.equal(frames[row, :count], alone)
        assert torch.equal(coefficients[row, :count], alone_coefficients)
        assert torch.equal(
            frames[row, count:], torch.zeros(10 - count, 512, device=device))
        assert (coefficients[row, count:] == 0).all()
    # lengths as a device tensor, out of range: clamped on the device
    clamped = harmonics.lpc(batch, torch.tensor(
        [-5, 256, 1100, 9999], dtype=torch.int32, device=device))
    assert torch.equal(clamped, frames)
    # a row that does not start on 16 bytes takes the scalar loads
    shifted = torch.zeros(2561, device=device)
    shifted[1:] = batch[3]
    assert shifted[1:].data_ptr() % 16 == 4
    assert torch.equal(harmonics.lpc(shifted[1:][None])[0], frames[3])
    # a strided batch is read in place
    wide = torch.zeros(4, 2600, device=device)
    wide[:, :2560] = batch
    assert torch.equal(harmonics.lpc_coefficients(
        wide[:, :2560], lengths=LENGTHS)[0], frames)


def test_graph_replay_with_other_lengths(device, ragged):
    batch = ragged.to(device)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=device)
    eager = harmonics.lpc(batch, lengths)               # warm: the tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = harmonics.lpc(batch, lengths)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    other = torch.tensor([2560, 700, 0, 1024], dtype=torch.int32,
                         device=device)
    batch[batch == 7.] = 0.                             # readable now
    want = harmonics.lpc(batch, other)
    lengths.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, want)
    assert not torch.equal(want, eager)


@pytest.fixture(scope='module')
def decoded(device, signals):
    audio = torch.from_numpy(signals[RESONANT])[None].to(device)
    pitch = torch.full((1, 8), 200.)
    return audio, pitch, {
        prior: harmonics.from_audio(
            audio, features='lpc', pitch=pitch if prior else None,
            return_features=True, _debug=True)
        for prior in (False, True)}


def test_peak_decoder_on_the_device_features(device, decoded):
    audio, _, _ = decoded
    contours, features = harmonics.from_audio(
        audio, features='lpc', decoder='peak', return_features=True)
    assert contours.shape == (3, 8) and features.shape == (512, 8)
    frames, frequencies = harmonics.lpc_coefficients(audio)
    assert torch.equal(features, frames.T)
    want = harmonics_oracle.peak_pick(
        features.T.cpu(), oracle.frequencies())
    assert same(contours.cpu(), want)
    # the envelope's first peaks are the three resonances (formants), to a
    # few bins of 21.6 Hz
    assert not want.isnan().any()
    centre = want.median(dim=1).values
    assert (centre - torch.tensor([700., 1800., 3200.])).abs().max() < 100.


@pytest.mark.parametrize('prior', [False, True])
def test_viterbi_decoder_on_the_device_features(device, decoded, prior):
    """Bin 0 is dropped: the decoder sees features[..., 1:] and
    frequencies[1:], and every round's path equals the oracle's decoder on
    the device's own observation, index for index"""
    _, pitch, runs = decoded
    contours, features, debug = runs[prior]
    assert contours.shape == (3, 8) and features.shape == (512, 8)
    assert torch.equal(features, debug['frames'][0].T)
    freqs = oracle.frequencies()[1:]
    transition = debug['transition'].dense().cpu().numpy()
    assert transition.shape == (511, 511) and not np.isnan(transition).any()
    initial = debug['initial'].cpu().numpy()
    rounds = 2 if prior else 3
    assert len(debug['observations']) == rounds
    first = 3 - rounds
    if prior:
        assert torch.equal(contours[0].cpu(), pitch[0])
    for round_, (x, indices, valid) in enumerate(zip(
            debug['observations'], debug['indices'], debug['valid'])):
        assert x.shape == (1, 8, 511)
        want = torch.from_numpy(harmonics_oracle.viterbi(
            x[0].cpu().numpy(), transition, initial, 8))
        assert torch.equal(indices[0].cpu(), want), round_
        assert valid.all()
        assert torch.equal(
            contours[first + round_].cpu(), freqs[want.long()])
    # what is decoded is bins 1 to 511 of the returned features on
    # frequencies[1:]: the first observation is, bit for bit, the observation
    # kernel's of that slice (a slice shifted by one bin, or the full
    # frequencies, gives another), and it is valid where the oracle's is
    sliced = features.T[None, :, 1:].contiguous()
    assert sliced.shape == (1, 8, 511)
    if prior:
        want_x, want_valid = harmonics.observation(
            sliced, freqs.to(device), pitch.to(device), 1. + .8,
            1. + 1. / .8)
    else:
        want_x, want_valid = harmonics.observation(sliced, freqs.to(device))
    assert torch.equal(debug['observations'][0], want_x)
    assert torch.equal(debug['valid'][0], want_valid)
    low, high = (1. + .8, 1. + 1. / .8) if prior else (None, None)
    oracle_x, oracle_valid = harmonics_oracle.observation(
        sliced[0].cpu(), freqs, pitch[0] if prior else None, low, high)
    assert torch.equal(want_valid[0].cpu(), oracle_valid)
    compared = (oracle_x > -80.) & ~want_x[0].cpu().isinf()
    assert compared.sum() >= 8 * (4 if prior else 100)
    # (fp32 rounding of scores up to 255, ulp 1.5e-5, is two orders under
    # this; a slice off by one bin is two orders over it)
    assert (want_x[0].cpu() - oracle_x)[compared].abs().max() < 1e-3
    assert not torch.equal(debug['observations'][0], harmonics.observation(
        features.T[None, :, :-1].contiguous(), freqs.to(device),
        *((pitch.to(device), 1. + .8, 1. + 1. / .8) if prior else ()))[0])
    # the model is the reference's expressions on frequencies[1:]. Its
    # unnormalised entries 1 - 3.5 |log2 f_i - log2 f_j| carry at most a few
    # ulp of log2 f <= 13.5 (9.5e-7 each) times 3.5 on either device, under
    # 2e-5; a row's sum is at least its diagonal, 1
    want_transition, want_initial = harmonics_oracle.decoder_model(freqs)
    assert (torch.from_numpy(np.exp(transition)) - want_transition
            ).abs().max() < 2e-5
    assert (torch.from_numpy(np.exp(initial)) - want_initial
            ).abs().max() < 1e-8
    assert np.isneginf(initial[-1]) and np.isfinite(initial[:-1]).all()
    if prior:
        assert (contours[1] >= 200. * 1.8 - 22.).all()
        assert (contours[1] <= 200. * 2.25 + 22.).all()


def test_nan_audio_gives_nan_frames_only_where_it_is_seen(device, signals):
    """NaN is a value here (-fhonor-nans): a NaN sample makes the frames
    whose window holds it NaN in every bin, and no other"""
    audio = torch.from_numpy(signals[RESONANT].copy())[None]
    audio[0, 1000] = float('nan')
    frames, _, coefficients = harmonics.lpc_coefficients(
        audio.to(device), return_coefficients=True)
    seen = [t for t in range(8) if 256 * t - 384 <= 1000 < 256 * t + 640]
    assert seen == [2, 3, 4, 5]
    clean, _ = harmonics.lpc_coefficients(
        torch.from_numpy(signals[RESONANT])[None].to(device))
    for t in range(8):
        if t in seen:
            assert frames[t].isnan().all()
            assert coefficients[t, 0] == 1
            assert coefficients[t, 1:].isnan().all()
        else:
            assert torch.equal(frames[t], clean[t])


def test_entries_and_error_paths(device, signals, tmp_path):
    import scipy.io.wavfile
    audio = torch.from_numpy(signals[RESONANT])[None]
    with pytest.raises(ValueError, match='librosa'):
        harmonics.from_audio(audio, features='lpc')
    with pytest.raises(ValueError, match='penn'):
        harmonics.from_audio(audio.to(device), features='posteriorgram')
    moved = harmonics.from_audio(audio, features='lpc', gpu=device.index)
    assert same(moved, harmonics.from_audio(audio.to(device), features='lpc'))
    assert harmonics.from_audio(
        audio.to(device), features='lpc', max_harmonics=1).shape == (1, 8)
    # a batch, ragged: each row is its stand-alone call
    batch = torch.cat([audio, audio.flip(1)]).to(device)
    both = harmonics.from_audio(batch, features='lpc', lengths=[2048, 1100])
    assert both.shape == (2, 3, 8)
    assert same(both[0], moved)
    assert same(both[1, :, :4], harmonics.from_audio(
        batch[1:, :1100], features='lpc'))
    assert both[1, :, 4:].isnan().all()
    # audio at another rate is resampled first
    doubled = promonet_amd.load.resample(audio.to(device), 22050, 44100)
    frames, _ = harmonics.lpc_coefficients(doubled, 44100)
    back = promonet_amd.load.resample(doubled, 44100, 22050)
    assert torch.equal(frames, harmonics.lpc_coefficients(back)[0])
    # the file entries take features=
    wav = tmp_path / 'voice.wav'
    pcm = (audio[0].numpy() * 32768).round().astype(np.int16)
    scipy.io.wavfile.write(wav, 22050, pcm)
    want, want_features = harmonics.from_audio(
        torch.from_numpy(pcm.astype(np.float32) / 32768)[None].to(device),
        features='lpc', return_features=True)
    harmonics.from_file_to_file(
        wav, tmp_path / 'harmonics.pt',
        output_feature_file=tmp_path / 'features.pt', gpu=device.index,
        features='lpc')
    assert same(torch.load(tmp_path / 'harmonics.pt'), want.cpu())
    assert torch.equal(torch.load(tmp_path / 'features.pt'),
                       want_features.cpu())

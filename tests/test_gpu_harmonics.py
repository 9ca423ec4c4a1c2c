"""promonet_amd.preprocess.harmonics stage by stage against the CPU
restatement of tests/harmonics_oracle.py, on a synthetic voice (harmonics 1-5
of a gliding f0) and a second, shorter row, as a ragged batch, and on the
small exact and edge inputs of the oracle (stft_cases, grid_inputs).

The high-pass is held bit for bit on a grid where fp32 is exact, and to the
oracle's own fp32 error on the voice. The STFT is held per bin to 4 x the
error of torch's own fp32 transform over the natural fp32 error model
(oracle.STFT_GATE). The observation is held to 4 x the oracle's own fp32
error. The decode is the exact link: each round's contour equals the oracle's
Viterbi run on the device's own observation, index for index.

Measured on an MI355X (printed by the tests): high-pass
error 0.81 x the oracle's fp32 recursion's (gate 4 x), and equal to the
integer recursion on the grid; STFT worst error per bin over the fp32 model
2 ** -24 * 12 * ||w x||_2 + 2 ** -23 * |X|: impulses 1.42, cosines 2.50,
shortest 0.58, ragged 2.54, rate16k 2.43, voice 3.35 (3.68 behind the device's
high-pass), fmax = 8000 3.99, where torch.stft in fp32 on the CPU has 5.03
(2.29 on MKL's AVX-512 path) and the gate is 20.12; observation error over the
oracle's own fp32 error 1.00 / 0.99 / 0.58 for round 0 / a masked round / the
prior path and at most 1.00 on the wide and edge windows (gate 4 x; the
kernel sums in float64 since [255, 257) at 700 states measured 5.66 in fp32);
contours within 2.69 Hz and 2.33 Hz of (k + 1) f0 (gate: one bin, 5.38 Hz).
"""
import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.preprocess import harmonics

import harmonics_oracle as oracle
import util

pytestmark = pytest.mark.gpu

SHORT = 9000


def same(a, b):
    """Bit-for-bit equality that lets NaN equal NaN"""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(), b.nan_to_num())


@pytest.fixture(scope='module')
def voices():
    audio, f0 = oracle.synthetic_voice()
    short, short_f0 = oracle.synthetic_voice(SHORT, glide=0., seed=1)
    batch = np.zeros((2, len(audio)), dtype=np.float32)
    batch[0] = audio
    batch[1, :SHORT] = short
    batch[1, SHORT:] = 7.                   # never read
    return torch.from_numpy(batch), [len(audio), SHORT], [f0, short_f0]


@pytest.fixture(scope='module')
def run(device, voices):
    batch, lengths, _ = voices
    contours, features, debug = harmonics.from_audio(
        batch.to(device), lengths=lengths, return_features=True, _debug=True)
    torch.cuda.synchronize()
    return contours, features, debug


def test_highpass(device, voices):
    batch, lengths, _ = voices
    x = batch[0, :8192]
    exact = oracle.biquad(x.numpy(), dtype=np.float64)
    single = oracle.biquad(x.numpy(), dtype=np.float32).astype(np.float64)
    got = harmonics.highpass(x[None].to(device), 22050, 1.33 * 50.)
    assert got.shape == (1, 8192) and got.dtype == torch.float32
    error = np.abs(got[0].cpu().numpy().astype(np.float64) - exact).max()
    reference = np.abs(single - exact).max()
    print(f'high-pass: device error {error:.3e}, fp32 recursion '
          f'{reference:.3e}, ratio {error / reference:.3f}')
    assert error <= 4 * reference
    # ragged: a row is filtered to its length and zero from there
    both = harmonics.highpass(
        batch[:, :8192].to(device), 22050, 1.33 * 50., lengths=[8192, 4099])
    assert torch.equal(both[0], got[0])
    alone = harmonics.highpass(
        batch[1:, :4099].to(device), 22050, 1.33 * 50.)
    assert torch.equal(both[1, :4099], alone[0])
    assert (both[1, 4099:] == 0).all()


def test_highpass_clamps_once_at_the_end(device):
    x = 4. * (-1.) ** np.arange(5000)
    x[2500:] *= .01
    free = oracle.biquad(x, clamp=False)
    assert np.abs(free).max() > 3.9
    got = harmonics.highpass(
        torch.from_numpy(x.astype(np.float32))[None].to(device), 22050,
        1.33 * 50.)[0].cpu().numpy()
    assert got.max() == 1. and got.min() == -1.
    # the state behind the clamp is the unclamped one
    np.testing.assert_allclose(got[2600:], free[2600:], atol=1e-4)
    assert np.abs(got[2600:]).max() < .05


@pytest.mark.parametrize('coefficients', oracle.GRID_COEFFICIENTS)
def test_highpass_is_exact_on_a_grid(device, coefficients):
    """Integer coefficients and inputs on a grid of 2^-12: every fma of the
    kernel is exact, so the output equals the integer recursion bit for bit.
    The row lengths sit around the 2048-sample chunks the state is carried
    across and end inside a quad of the recursion; lengths below 0 and above
    the row are clamped; the row strides are not the row length."""
    X = oracle.grid_inputs()
    rows, n = X.shape
    lengths = torch.tensor(oracle.GRID_LENGTHS, dtype=torch.int32)
    clamped = lengths.clamp(0, n).tolist()
    assert rows == len(clamped) and max(clamped) == n and min(clamped) == 0
    for scale in (oracle.GRID_SCALE, oracle.GRID_CLAMPING_SCALE):
        x = torch.full((rows, n + 3), float('nan'))
        x[:, :n] = torch.from_numpy(X * scale)
        x, row_lengths = x.to(device), lengths.to(device)
        y = torch.full((rows, n + 5), -77., device=device)
        _lib.check(_lib.lib().pm_harmonics_highpass(
            _lib.ptr(x), _lib.ptr(row_lengths, torch.int32), _lib.ptr(y),
            rows, n, n + 3, n + 5, *(float(c) for c in coefficients),
            _lib.stream()))
        y = y.cpu()
        assert (y[:, n:] == -77.).all()
        released = 0
        for row, length in enumerate(clamped):
            free = oracle.biquad_grid(X[row, :length], coefficients, scale)
            want = torch.from_numpy(np.clip(free, -1, 1)).to(torch.float32)
            # (float32 holds the oracle's values exactly)
            assert np.array_equal(want.double().numpy(), np.clip(free, -1, 1))
            assert torch.equal(y[row, :length], want), (scale, row, length)
            assert (y[row, length:n] == 0).all(), (scale, row)
            over = np.abs(free) > 1
            if over.any():
                # the state behind the clamp is the unclamped one
                after = np.flatnonzero(~over[np.argmax(over):]) + \
                    np.argmax(over)
                assert torch.equal(
                    y[row, after], torch.from_numpy(free[after]).float())
                released += len(after)
        assert (released > 0) == (scale == oracle.GRID_CLAMPING_SCALE)


def test_stft(device, voices):
    batch, lengths, _ = voices
    filtered = harmonics.highpass(
        batch.to(device), 22050, 1.33 * 50., lengths=lengths)
    frames, frequencies, counts = harmonics.magnitude(
        filtered, lengths, 22050, 50.)
    want_frequencies, minidx = oracle.frequencies()
    assert minidx == 10
    assert torch.equal(frequencies.cpu(), want_frequencies)
    assert frames.shape == (2, 22150 // 256, 2039)
    assert counts.tolist() == [22150 // 256, SHORT // 256]
    assert (frames[1, SHORT // 256:] == 0).all()
    for row, length in enumerate(lengths):
        want, _, l2 = oracle.stft(filtered[row, :length].cpu())
        count = length // 256
        assert want.shape == (count, 2039)
        figure = oracle.stft_figure(frames[row, :count].cpu(), want, l2)
        print(f'STFT: row {row}: error over the fp32 model {figure:.3f} '
              f'(gate {oracle.STFT_GATE[0]:.2f})')
        util.check(figure, oracle.STFT_GATE[0], 'harmonics/stft',
                   f'voice row {row}')
    # the public entry: high-pass and transform, (T, S) for one recording
    single, freqs = harmonics.stft(batch[:1].to(device))
    assert torch.equal(single, frames[0]) and torch.equal(freqs, frequencies)
    with pytest.raises(ValueError, match='too short'):
        harmonics.stft(batch[:1, :1920].to(device))
    harmonics.stft(batch[:1, :1921].to(device))


@pytest.mark.parametrize(
    'case', ['impulses', 'cosines', 'shortest', 'ragged', 'rate16k', 'voice'])
def test_stft_per_bin(device, case):
    """Every bin of every frame within 4 x the error of torch's own fp32
    transform (oracle.STFT_GATE), at geometries the pipeline's voice never
    reaches: bin0 = 0 with DC and Nyquist, both reflections in one frame,
    hop 185 with three paddings, ragged rows"""
    audio, lengths, rate, fmin, counts = oracle.stft_cases()[case]
    x = audio.to(device)
    frames, frequencies, got_counts = harmonics.magnitude(
        x, lengths, rate, fmin, counts)
    wanted = oracle.stft_case_oracle(case)
    want_frequencies, minidx = oracle.frequencies(rate, fmin)
    assert torch.equal(frequencies.cpu(), want_frequencies)
    assert got_counts.dtype == torch.int32
    assert got_counts.tolist() == [len(want) for want, _, _ in wanted]
    assert frames.shape == (
        len(lengths), max(got_counts.tolist()), 2049 - minidx)
    figures = []
    for row, (want, _, l2) in enumerate(wanted):
        got = frames[row, :len(want)].cpu()
        assert got.shape == want.shape
        assert (frames[row, len(want):] == 0).all()
        figures.append(oracle.stft_figure(got, want, l2))
        assert figures[-1] == figures[-1], (case, row)          # no NaN
    print(f'STFT {case}: error over the fp32 model {max(figures):.3f}, '
          f'torch.stft in fp32 {oracle.stft_fp32_figure(case):.3f} '
          f'(gate {oracle.STFT_GATE[0]:.2f})')
    util.check(max(figures), oracle.STFT_GATE[0], 'harmonics/stft', case)
    # each row of a batch equals its stand-alone call bit for bit
    if len(lengths) > 1:
        for row, length in enumerate(lengths):
            alone, _, alone_counts = harmonics.magnitude(
                x[row:row + 1, :length].contiguous(), [length], rate, fmin,
                None if counts is None else counts[row:row + 1])
            count = len(wanted[row][0])
            assert alone_counts.tolist() == [count]
            assert torch.equal(alone[0], frames[row, :count]), (case, row)


def test_stft_at_another_rate(device, voices):
    """fmax = 8000: the high-pass, the resampler to 16 kHz and the transform
    at hop 185 with the frame count of the recording at 22 050 Hz"""
    batch, _, _ = voices
    audio = batch[1:, :SHORT].to(device)
    frames, frequencies = harmonics.stft(audio, fmax=8000)
    filtered = harmonics.highpass(audio, 22050, 1.33 * 50., lengths=[SHORT])
    resampled, lengths = promonet_amd.load.resample(
        filtered, 22050, 16000, lengths=[SHORT])
    assert lengths == [6531]
    by_hand, by_hand_frequencies, counts = harmonics.magnitude(
        resampled.contiguous(), lengths, 16000, 50., [SHORT // 256])
    assert torch.equal(frames, by_hand[0])
    assert torch.equal(frequencies, by_hand_frequencies)
    # the oracle at this geometry, on the device's own resampled audio
    want, _, l2 = oracle.stft(
        resampled[0, :6531].cpu(), 16000, 50., SHORT // 256)
    want_frequencies, minidx = oracle.frequencies(16000, 50.)
    # (34 frames come out where the recording has 35 at 22 050 Hz: the
    # reference's geometry, kept)
    assert oracle.stft_geometry(6531, 16000, SHORT // 256) == (185, 1920, 34)
    assert minidx == 13 and frames.shape == want.shape == (34, 2036)
    assert counts.tolist() == [34]
    assert torch.equal(frequencies.cpu(), want_frequencies)
    figure = oracle.stft_figure(frames.cpu(), want, l2)
    print(f'STFT at 16 kHz: error over the fp32 model {figure:.3f} '
          f'(gate {oracle.STFT_GATE[0]:.2f})')
    util.check(figure, oracle.STFT_GATE[0], 'harmonics/stft', '16 kHz')


def check_observation(got, valid, features, freqs, f0=None, low=None,
                      high=None, every=False):
    """-> measured error over the oracle's own fp32 error (0 where both are
    exact). every: no entry inside a valid frame's window may be left out
    of the comparison."""
    want, want_valid = oracle.observation(features, freqs, f0, low, high)
    exact, _ = oracle.observation(
        features, freqs, f0, low, high, dtype=torch.float64)
    got, valid = got.cpu(), valid.cpu()
    assert torch.equal(valid, want_valid)
    assert (got[~valid] == 0).all()
    states = features.shape[-1]
    inside = torch.ones_like(got, dtype=torch.bool)
    if f0 is not None:
        lo = torch.searchsorted(freqs, f0 * low)
        hi = torch.searchsorted(freqs, f0 * high)
        index = torch.arange(states)[None]
        inside = (index >= lo[:, None]) & (index < hi[:, None])
    inside &= valid[:, None]
    outside = ~inside & valid[:, None]
    assert (got[outside] == -float('inf')).all()
    differs = got.isinf() != want.isinf()
    assert (want[differs & inside] < -87.3).all()
    compared = inside & ~got.isinf() & ~want.isinf() & (want >= -87.3)
    assert compared.any()
    assert not every or torch.equal(compared, inside)
    error = (got.to(torch.float64) - exact)[compared].abs().max().item()
    reference = (want.to(torch.float64) - exact)[compared].abs().max().item()
    assert error <= 4 * reference, (error, reference)
    return error / reference if reference else 0.


def test_observation(device, voices, run):
    _, _, f0s = voices
    contours, _, debug = run
    features = debug['frames'][0].contiguous()          # (T, S), row 0
    freqs = debug['frequencies']
    count = features.shape[0]
    ratios = {}
    got, valid = harmonics.observation(features[None], freqs)
    ratios['round 0'] = check_observation(
        got[0], valid[0], features.cpu(), freqs.cpu())
    # a masked round on the decoded f0, with a NaN f0 and an empty mask
    f0 = contours[0, 0].clone()
    f0[3] = float('nan')
    f0[5] = 1e6
    f0[7] = 1.                                          # below every bin
    got, valid = harmonics.observation(
        features[None], freqs, f0[None].contiguous(), 2 + .8, 2 + 1 / .8)
    assert valid[0].cpu().tolist() == [
        i not in (3, 5, 7) for i in range(count)]
    ratios['masked'] = check_observation(
        got[0], valid[0], features.cpu(), freqs.cpu(), f0.cpu(), 2 + .8,
        2 + 1 / .8)
    # the prior path's first mask
    centres = 256 * np.arange(count) + 128
    pitch = torch.from_numpy(f0s[0][centres].astype(np.float32))
    got, valid = harmonics.observation(
        features[None], freqs, pitch[None].to(device), 1. + .8, 1. + 1. / .8)
    ratios['prior'] = check_observation(
        got[0], valid[0], features.cpu(), freqs.cpu(), pitch, 1. + .8,
        1. + 1. / .8)
    # frames past a row's count are zeros and not valid
    got, valid = harmonics.observation(
        features[None], freqs, lengths=torch.tensor([4]))
    assert (got[0, 4:] == 0).all() and not valid[0, 4:].any()
    assert valid[0, :4].all()
    print('observation: error / oracle fp32 error ' + ', '.join(
        f'{key} {value:.3f}' for key, value in ratios.items()))


def mask_windows():
    """(states, first, last): all of the row, its first and its last bin
    alone, one across the first pass of 256 threads, one wider than two
    passes"""
    windows = []
    for states in (1, 255, 256, 257, 700):
        windows += [(states, 0, states), (states, 0, 1),
                    (states, states - 1, states)]
        if states >= 257:
            windows.append((states, 255, 257))
        if states == 700:
            windows.append((states, 100, 650))
    return list(dict.fromkeys(windows))


@pytest.mark.parametrize('states,first,last', mask_windows())
def test_observation_with_wide_and_edge_masks(device, states, first, last):
    """Masked windows the voice never has, in five frames; the sixth frame's
    window is empty. Features in [0, 8] keep log softmax above -(8 + ln 700):
    every inside entry is compared.

    [700-255-257] is the case that moved the kernel's sum to float64: composed
    in fp32 (expf, a division, logf) the device was one ulp, 4.81e-7, off at
    an entry of -6.13, 5.66 x the oracle's own fp32 error of 8.50e-8 over the
    ten entries of that window."""
    generator = torch.Generator().manual_seed(states)
    features = 8. * torch.rand(6, states, generator=generator)
    # freqs[s] = s + 1: searchsorted(freqs, s + 0.5) = s
    freqs = torch.arange(1., states + 1.)
    f0 = torch.tensor([1., 1., 1., 1., 1., 1e6])
    low, high = first + .5, last + .5
    lo = torch.searchsorted(freqs, f0 * low).tolist()
    hi = torch.searchsorted(freqs, f0 * high).tolist()
    assert lo == [first] * 5 + [states] and hi == [last] * 5 + [states]
    got, valid = harmonics.observation(
        features[None].to(device), freqs.to(device), f0[None].to(device),
        low, high)
    assert valid[0].tolist() == [True] * 5 + [False]
    ratio = check_observation(
        got[0], valid[0], features, freqs, f0, low, high, every=True)
    print(f'observation, {states} states, [{first}, {last}): error / oracle '
          f'fp32 error {ratio:.3f}')


def test_decode_equals_the_oracle_on_the_device_observation(run):
    contours, _, debug = run
    transition = debug['transition'].dense().cpu().numpy()
    initial = debug['initial'].cpu().numpy()
    freqs = debug['frequencies'].cpu()
    counts = debug['counts'].tolist()
    assert len(debug['observations']) == 3
    for round_, (x, indices, valid) in enumerate(zip(
            debug['observations'], debug['indices'], debug['valid'])):
        for row, count in enumerate(counts):
            want = torch.from_numpy(oracle.viterbi(
                x[row].cpu().numpy(), transition, initial, count))
            assert torch.equal(indices[row].cpu(), want), (round_, row)
            assert valid[row, :count].all() and not valid[row, count:].any()
            assert torch.equal(
                contours[row, round_, :count].cpu(), freqs[want[:count].long()])
            assert contours[row, round_, count:].isnan().all()


def test_end_to_end(device, voices, run):
    batch, lengths, f0s = voices
    contours, features, debug = run
    count = lengths[0] // 256
    assert contours.shape == (2, 3, count) and contours.is_cuda
    assert features.shape == (2, 2039, count)
    for row, length in enumerate(lengths):
        worst = oracle.check_contours(
            contours[row, :, :length // 256].cpu(), f0s[row])
        print(f'row {row}: worst distance from (k + 1) f0 {worst:.2f} Hz')
        assert worst <= oracle.BIN
    # one recording: (max_harmonics, frames) and features (S, T)
    alone, alone_features = harmonics.from_audio(
        batch[:1], return_features=True, gpu=device.index)
    assert alone.shape == (3, count) and alone_features.shape == (2039, count)
    assert same(alone, contours[0])
    assert torch.equal(alone_features, features[0])
    # each ragged row equals its stand-alone call
    short = harmonics.from_audio(batch[1:, :SHORT].to(device))
    assert same(short, contours[1, :, :SHORT // 256])
    assert harmonics.from_audio(
        batch[:1].to(device), max_harmonics=1).shape == (1, count)
    # the prior becomes harmonic 0
    centres = 256 * np.arange(count) + 128
    pitch = torch.from_numpy(f0s[0][centres].astype(np.float32))[None]
    prior = harmonics.from_audio(batch[:1].to(device), pitch=pitch)
    assert torch.equal(prior[0].cpu(), pitch[0])
    assert oracle.check_contours(prior.cpu(), f0s[0]) <= oracle.BIN
    # audio at another rate is resampled first
    doubled = promonet_amd.load.resample(batch[:1].to(device), 22050, 44100)
    again = harmonics.from_audio(doubled, 44100)
    assert again.shape == (3, count)
    assert oracle.check_contours(again.cpu(), f0s[0]) <= oracle.BIN


def test_peak_pick(device, run):
    frames = torch.tensor([
        [0, 1, 0, 2, 2, 2, 0, 3, 3, 4, 4, 1],       # plateaus
        [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0],       # the last interior bin
        [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5],       # none
        [0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 3],       # more than three
        [1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2]],      # a plateau to the edge
        dtype=torch.float32)
    freqs = 10. * torch.arange(12.) + 3.
    want = oracle.peak_pick(frames, freqs)
    assert want[:, 0].tolist() == [13., 43., 93.]
    assert want[0, 1] == 103. and want[1:, 1].isnan().all()
    assert want[:, 2].isnan().all() and want[:, 3].tolist() == [13., 33., 53.]
    got = harmonics.peak_pick(frames.to(device), freqs.to(device))
    assert got.shape == (3, 5) and same(got.cpu(), want)
    generator = torch.Generator().manual_seed(0)
    noise = torch.randint(0, 4, (2, 40, 67), generator=generator).float()
    got = harmonics.peak_pick(
        noise.to(device), torch.arange(67.), max_harmonics=5)
    assert got.shape == (2, 5, 40)
    for row in range(2):
        assert same(got[row].cpu(),
                    oracle.peak_pick(noise[row], torch.arange(67.), 5))
    # the decoder of from_audio, on the device's features
    _, _, debug = run
    features, counts = debug['frames'], debug['counts'].tolist()
    picked = harmonics.peak_pick(
        features, debug['frequencies'], lengths=debug['counts'])
    for row, count in enumerate(counts):
        assert same(picked[row, :, :count].cpu(), oracle.peak_pick(
            features[row, :count].cpu(), debug['frequencies'].cpu()))
        assert picked[row, :, count:].isnan().all()


def test_file_entries(device, voices, run, tmp_path):
    import scipy.io.wavfile
    batch, lengths, _ = voices
    gpu = device.index
    loudness, contours = promonet_amd.preprocess.from_audio(
        batch[:1], gpu=gpu, features=['loudness', 'harmonics'])
    assert loudness.shape == (promonet_amd.LOUDNESS_BANDS, lengths[0] // 256)
    assert same(contours, run[0][0])
    only = promonet_amd.preprocess.from_audio(
        batch[:1], gpu=gpu, features=['harmonics'], max_harmonics=2)
    assert same(only, run[0][0, :2])

    wav = tmp_path / 'voice.wav'
    pcm = (batch[0].numpy() * 32768).round().astype(np.int16)
    scipy.io.wavfile.write(wav, 22050, pcm)
    want = harmonics.from_audio(
        torch.from_numpy(pcm.astype(np.float32) / 32768)[None].to(device))
    promonet_amd.preprocess.from_file_to_file(
        wav, tmp_path / 'a', gpu=gpu, features=['loudness', 'harmonics'])
    assert (tmp_path / 'a-loudness.pt').exists()
    assert same(torch.load(tmp_path / 'a-harmonics.pt'), want.cpu())
    promonet_amd.preprocess.from_files_to_files(
        [wav], [tmp_path / 'b'], gpu=gpu, features=['harmonics'])
    assert same(torch.load(tmp_path / 'b-harmonics.pt'), want.cpu())
    assert torch.load(tmp_path / 'b-harmonicfeatures.pt').shape == \
        (2039, lengths[0] // 256)
    # the module's own file entries, with a pitch prior from a file
    pitch = torch.full((1, lengths[0] // 256), 120.)
    torch.save(pitch, tmp_path / 'c-pitch.pt')
    harmonics.from_files_to_files(
        [wav], [tmp_path / 'c-harmonics.pt'],
        pitch_files=[tmp_path / 'c-pitch.pt'],
        output_feature_files=[tmp_path / 'c-features.pt'], gpu=gpu)
    saved = torch.load(tmp_path / 'c-harmonics.pt')
    assert saved.shape == (3, lengths[0] // 256)
    assert torch.equal(saved[0], pitch[0]) and not saved[1:].isnan().any()
    assert torch.load(tmp_path / 'c-features.pt').shape == \
        (2039, lengths[0] // 256)

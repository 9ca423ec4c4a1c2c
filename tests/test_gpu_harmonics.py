"""promonet_amd.preprocess.harmonics stage by stage against the CPU
restatement of tests/harmonics_oracle.py, on a synthetic voice (harmonics 1-5
of a gliding f0) and a second, shorter row, as a ragged batch.

The arithmetic stages are held to bounds computed here from the oracle's own
fp32 error; the decode is the exact link: each round's contour equals the
oracle's Viterbi run on the device's own observation, index for index.

Measured on an MI355X (printed by the tests): high-pass
error 0.81 x the oracle's fp32 recursion's (gate 4 x); STFT worst error 0.0006
of the direct-sum bound; observation error over the oracle's own fp32 error
1.00 / 2.88 / 1.74 for round 0 / a masked round / the prior path (gate 4 x);
contours within 2.69 Hz and 2.33 Hz of (k + 1) f0 (gate: one bin, 5.38 Hz).
"""
import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd.preprocess import harmonics

import harmonics_oracle as oracle

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
    worst = 0.
    for row, length in enumerate(lengths):
        want, scale = oracle.stft(filtered[row, :length].cpu())
        count = length // 256
        assert want.shape == (count, 2039)
        bound = (4096 + 2) * 2. ** -24 * scale[:, None] + 2. ** -22 * want
        error = (frames[row, :count].cpu().to(torch.float64) - want).abs()
        worst = max(worst, (error / bound).max().item())
        assert (error <= bound).all(), (row, (error / bound).max().item())
    print(f'STFT: worst error / bound {worst:.4f}')
    # the public entry: high-pass and transform, (T, S) for one recording
    single, freqs = harmonics.stft(batch[:1].to(device))
    assert torch.equal(single, frames[0]) and torch.equal(freqs, frequencies)
    with pytest.raises(ValueError, match='too short'):
        harmonics.stft(batch[:1, :1920].to(device))
    harmonics.stft(batch[:1, :1921].to(device))


def check_observation(got, valid, features, freqs, f0=None, low=None,
                      high=None):
    """-> measured error over the oracle's own fp32 error"""
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
    error = (got.to(torch.float64) - exact)[compared].abs().max().item()
    reference = (want.to(torch.float64) - exact)[compared].abs().max().item()
    assert error <= 4 * reference, (error, reference)
    return error / reference


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

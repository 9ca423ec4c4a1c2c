"""The harmonics oracle (tests/harmonics_oracle.py), the band packing of
promonet_amd.viterbi and the surface of the new modules. No GPU."""
import ctypes
import inspect
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd import _lib, viterbi
from promonet_amd.preprocess import harmonics

import harmonics_oracle as oracle


@pytest.mark.parametrize('states,frames', [(1, 3), (2, 5), (3, 4), (4, 5)])
def test_viterbi_oracle_finds_the_brute_force_optimum(states, frames):
    generator = torch.Generator().manual_seed(states * 10 + frames)
    for _ in range(5):
        observation = torch.randn(frames, states, generator=generator).numpy()
        transition = torch.randn(states, states, generator=generator).numpy()
        initial = torch.randn(states, generator=generator).numpy()
        path = oracle.viterbi(observation, transition, initial)
        assert path.dtype == np.int32 and path.shape == (frames,)
        got = oracle.path_score(path, observation, transition, initial)
        want = oracle.brute_force(observation, transition, initial)
        assert got == want


def test_viterbi_oracle_ties_and_lengths():
    # everything equal: the lowest index everywhere; all -inf alike
    for value in (0., -float('inf')):
        observation = np.full((4, 3), value, dtype=np.float32)
        path = oracle.viterbi(
            observation, np.zeros((3, 3), np.float32), np.zeros(3, np.float32))
        assert path.tolist() == [0, 0, 0, 0]
    # transition[j, i] is the step from i to j: from state 0 only 1 is open
    ninf = -float('inf')
    transition = np.array([[ninf, ninf], [0., ninf]], dtype=np.float32)
    observation = np.zeros((2, 2), dtype=np.float32)
    initial = np.array([0., ninf], dtype=np.float32)
    assert oracle.viterbi(observation, transition, initial).tolist() == [0, 1]
    assert oracle.viterbi(
        observation, transition, initial, length=1).tolist() == [0, 0]


def harmonic_transition(states):
    freqs = oracle.BIN * (10 + torch.arange(states, dtype=torch.float32))
    with np.errstate(divide='ignore'):
        return torch.log(oracle.decoder_model(freqs)[0])


def interior_transition(states, seed=0):
    """A band with -inf inside its ranges, an empty row and a full row"""
    generator = torch.Generator().manual_seed(seed)
    matrix = -torch.randint(0, 33, (states, states), generator=generator) / 8.
    index = torch.arange(states)
    far = (index[:, None] - index[None]).abs() > max(2, states // 5)
    matrix[far] = -float('inf')
    holes = torch.rand(states, states, generator=generator) < .3
    matrix[holes] = -float('inf')
    if states > 3:
        matrix[1] = -float('inf')
        matrix[2] = -.5
    return matrix


@pytest.mark.parametrize('states', [1, 2, 5, 64, 257])
def test_band_packing_round_trips(states):
    generator = torch.Generator().manual_seed(states)
    dense = torch.randn(states, states, generator=generator)
    for matrix in (dense, harmonic_transition(states),
                   interior_transition(states)):
        packed = viterbi.Transition(matrix, log_probs=True)
        lo, count, offset = packed.table.to(torch.int64)
        assert packed.table.dtype == torch.int32
        assert packed.table.shape == (3, states)
        assert packed.band.dtype == torch.float32
        assert (offset % 4 == 0).all() and packed.band.numel() % 4 == 0
        assert (lo >= 0).all() and (lo + count <= states).all()
        assert int(offset[-1] + (count[-1] + 3) // 4 * 4) == \
            packed.band.numel()
        assert torch.equal(packed.dense(), matrix)
        # the range holds every finite entry and starts and ends on one
        finite = matrix > -float('inf')
        for row in range(states):
            where = finite[row].nonzero()[:, 0]
            if len(where):
                assert lo[row] == where[0] and count[row] == \
                    where[-1] + 1 - where[0]
            else:
                assert count[row] == 0
    assert (viterbi.Transition(dense, True).table[1] == states).all()
    # probabilities are logged: zeros leave the band
    packed = viterbi.Transition(torch.eye(states))
    assert (packed.table[1] == 1).all()
    assert torch.equal(packed.dense(), torch.log(torch.eye(states)))


def test_harmonic_band_is_sparse():
    freqs, minidx = oracle.frequencies()
    assert minidx == 10 and len(freqs) == 2039
    transition, initial = oracle.decoder_model(freqs)
    packed = viterbi.Transition(transition)
    finite = int((transition > 0).sum())
    assert finite == 753919
    assert finite <= packed.band.numel() <= finite + 3 * 2039 + 2039
    assert packed.band.numel() * 4 < 4 * 1024 * 1024     # one XCD's L2


@pytest.fixture(scope='module')
def voice():
    audio, f0 = oracle.synthetic_voice()
    return audio, f0, oracle.from_audio(audio)


def test_oracle_tracks_a_synthetic_voice(voice):
    audio, f0, contours = voice
    assert contours.shape == (3, 22150 // 256)
    worst = oracle.check_contours(contours, f0)
    print(f'worst distance from (k + 1) f0: {worst:.2f} Hz')
    assert worst <= oracle.BIN


def test_oracle_tracks_a_flat_voice_and_takes_a_prior():
    audio, f0 = oracle.synthetic_voice(glide=0.)
    contours = oracle.from_audio(audio)
    assert oracle.check_contours(contours, f0) <= oracle.BIN
    count = contours.shape[-1]
    pitch = torch.full((1, count), 110.)
    prior = oracle.from_audio(audio, pitch=pitch)
    assert torch.equal(prior[0], pitch[0])
    assert oracle.check_contours(prior, f0) <= oracle.BIN


def test_oracle_biquad_and_peaks():
    # a high-pass: DC goes, the Nyquist alternation stays
    y = oracle.biquad(np.ones(4000))
    assert abs(y[-1]) < 1e-6
    y = oracle.biquad(.5 * (-1.) ** np.arange(4000))
    assert abs(abs(y[-1]) - .5) < 1e-3
    # clamped once, at the end
    assert oracle.biquad(4. * (-1.) ** np.arange(64)).max() == 1.
    x = np.array([0, 1, 0, 2, 2, 2, 0, 3, 3, 4, 4, 1, 5], dtype=np.float32)
    assert oracle.find_peaks(x).tolist() == [1, 4, 9]
    scipy_signal = pytest.importorskip('scipy.signal')
    generator = np.random.RandomState(0)
    for _ in range(20):
        x = generator.randint(0, 4, 50).astype(np.float32)
        assert oracle.find_peaks(x).tolist() == \
            scipy_signal.find_peaks(x)[0].tolist()


def test_stft_gate_is_four_times_the_fp32_figure():
    """MKL chooses its transform by the processor, so the figure is taken in
    a child process on the code path that every processor has"""
    script = (
        'import json, sys\n'
        f'sys.path.insert(0, {str(Path(__file__).parent)!r})\n'
        'import harmonics_oracle as oracle\n'
        'print(json.dumps({name: oracle.stft_fp32_figure(name) '
        'for name in oracle.stft_cases()}))\n')
    environment = dict(
        os.environ, MKL_CBWR='COMPATIBLE', OMP_NUM_THREADS='1',
        MKL_NUM_THREADS='1')
    output = subprocess.run(
        [sys.executable, '-c', script], env=environment, check=True,
        capture_output=True, text=True).stdout
    figures = json.loads(output.splitlines()[-1])
    print('fp32 torch.stft over the natural error model: ' + ', '.join(
        f'{name} {figure:.2f}' for name, figure in figures.items()))
    assert list(figures) == [
        'impulses', 'cosines', 'shortest', 'ragged', 'rate16k', 'voice']
    assert round(max(figures.values()), 2) == oracle.STFT_GATE[1] == 5.03
    assert oracle.STFT_GATE[0] == 4 * oracle.STFT_GATE[1]
    # whatever path this process takes, its figure is within the gate
    here = max(oracle.stft_fp32_figure(name) for name in figures)
    print(f'in this process: {here:.2f}')
    assert 0 < here < oracle.STFT_GATE[0]


def test_stft_cases_have_the_geometry_they_are_named_for():
    cases = oracle.stft_cases()
    for name, (audio, lengths, target_rate, fmin, counts) in cases.items():
        assert audio.dtype == torch.float32 and audio.shape[0] == len(lengths)
        assert audio.shape[1] == max(lengths)
        for row, length in zip(oracle.stft_case_rows(name), lengths):
            _, size, count = oracle.stft_geometry(length, row[1], row[3])
            assert 0 <= size < length and count >= 1
    assert oracle.frequencies(22050, 0.)[1] == 0
    assert oracle.stft_case_oracle('cosines')[0][0].shape == (19, 2049)
    assert oracle.stft_geometry(1921) == (256, 1920, 7)
    audio, lengths, target_rate, fmin, counts = cases['rate16k']
    assert oracle.frequencies(16000, fmin)[1] == 13
    geometry = [oracle.stft_geometry(length, 16000, count)
                for length, count in zip(lengths, counts)]
    assert [item[:2] for item in geometry] == [
        (185, 1920), (185, 1550), (185, 2197)]
    assert all(item[1] < length for item, length in zip(geometry, lengths))
    assert [len(want) for want, _, _ in oracle.stft_case_oracle('rate16k')] \
        == [item[2] for item in geometry]
    # a tone on bin k0 peaks there at amplitude x sum(w) / 2 = 0.5 x 1024
    for row, k0 in enumerate((10, 11, 1000, 2047)):
        want = oracle.stft_case_oracle('cosines')[row][0][9]
        assert int(want.argmax()) == k0 and abs(want[k0] - 512.) < .01
    dc, nyquist = (oracle.stft_case_oracle('cosines')[row][0][9]
                   for row in (4, 5))
    assert abs(dc[0] - 512.) < .01 and abs(nyquist[2048] - 512.) < .01


def test_stft_gate_is_tighter_than_the_direct_sum_bound_at_every_bin():
    """4 x 5.03 (12 L2 + 2 |X|) against 4098 L1 + 4 |X| (units of 2^-24):
    L2 <= L1 and |X| <= L1 + 1e-3"""
    for want, scale, l2 in oracle.stft_case_oracle('voice'):
        before = (4096 + 2) * 2. ** -24 * scale[:, None] + 2. ** -22 * want
        now = oracle.STFT_GATE[0] * oracle.stft_model(want, l2)
        assert (now < before).all()
        print(f'direct-sum bound over the gated model: median '
              f'{(before / now).median().item():.0f}')


def stft_before(filtered):
    """oracle.stft as it stood before it took a geometry"""
    audio = torch.as_tensor(filtered, dtype=torch.float64)[None]
    frames = audio.shape[-1] // 256
    size = 256 * (frames - (audio.shape[-1] // 256)) // 2 + (4096 - 256) // 2
    audio = torch.nn.functional.pad(audio[None], (size, size), 'reflect')[0]
    window = torch.hann_window(4096, dtype=torch.float64)
    result = torch.view_as_real(torch.stft(
        audio, 4096, hop_length=256, window=window, center=False,
        normalized=False, onesided=True, return_complex=True))
    spectrogram = torch.sqrt(result.pow(2).sum(-1) + 1e-6)
    scale = (audio[0].unfold(0, 4096, 256) * window).abs().sum(-1)
    return spectrogram[0][10:].T.contiguous(), scale


def test_stft_defaults_are_unchanged():
    audio, lengths = oracle.stft_cases()['voice'][:2]
    for row, length in enumerate(lengths):
        want, scale, l2 = oracle.stft(audio[row, :length])
        before, before_scale = stft_before(audio[row, :length])
        assert torch.equal(want, before) and torch.equal(scale, before_scale)
        assert want.dtype == torch.float64 and l2.shape == scale.shape
        assert (l2 <= scale).all() and (l2 > 0).all()
        assert torch.equal(want, oracle.stft_case_oracle('voice')[row][0])


def test_biquad_grid_is_the_float64_recursion_and_fits_fp32():
    X = oracle.grid_inputs()
    assert X.shape == (len(oracle.GRID_LENGTHS), oracle.GRID_SAMPLES)
    assert X.min() == -8 and X.max() == 8
    for coefficients in oracle.GRID_COEFFICIENTS:
        above = below_again = total = 0
        for row, length in zip(X, oracle.GRID_LENGTHS):
            row = row[:max(0, min(length, oracle.GRID_SAMPLES))]
            y, peak = oracle.biquad_grid(row, coefficients, return_peak=True)
            assert peak < 2 ** 24
            assert np.array_equal(y, oracle.biquad(
                row * oracle.GRID_SCALE, coefficients, clamp=False))
            assert np.array_equal(y, oracle.biquad(
                (row * oracle.GRID_SCALE).astype(np.float32), coefficients,
                dtype=np.float32, clamp=False))
            if len(y):
                assert np.abs(y).max() < 1
            free = oracle.biquad_grid(
                row, coefficients, oracle.GRID_CLAMPING_SCALE)
            clamped = oracle.biquad_grid(
                row, coefficients, oracle.GRID_CLAMPING_SCALE, clamp=True)
            assert np.array_equal(clamped, oracle.biquad(
                row * oracle.GRID_CLAMPING_SCALE, coefficients))
            assert np.array_equal(clamped, np.clip(free, -1, 1))
            over = np.abs(free) > 1
            total += len(free)
            above += int(over.sum())
            if over.any():
                below_again += int((~over[np.argmax(over):]).sum())
        print(f'{coefficients}: {above} of {total} samples clamp, '
              f'{below_again} below 1 after the first that does')
        assert above >= .01 * total and below_again >= .01 * total


def test_module_surface():
    assert promonet_amd.MAX_HARMONICS == 3
    assert promonet_amd.config.MAX_HARMONICS == 3
    names = list(inspect.signature(harmonics.from_audio).parameters)
    assert names[:8] == [
        'audio', 'sample_rate', 'pitch', 'features', 'decoder',
        'max_harmonics', 'return_features', 'gpu']
    assert 'lengths' in names
    parameters = inspect.signature(harmonics.from_audio).parameters
    assert parameters['features'].default == 'stft'
    assert parameters['decoder'].default == 'viterbi'
    for name in ('from_file', 'from_file_to_file', 'from_files_to_files',
                 'stft', 'viterbi', 'peak_pick'):
        assert callable(getattr(harmonics, name)), name
    assert list(inspect.signature(harmonics.from_files_to_files).parameters) \
        == ['files', 'output_files', 'pitch_files', 'output_feature_files',
            'max_harmonics', 'gpu']
    assert list(inspect.signature(viterbi.from_probabilities).parameters) == [
        'observation', 'batch_frames', 'transition', 'initial', 'log_probs']
    assert 'unpinned' in viterbi.__doc__

    audio = torch.zeros(1, 4096)
    with pytest.raises(ValueError, match='librosa'):
        harmonics.from_audio(audio, features='lpc')
    with pytest.raises(ValueError, match='penn'):
        harmonics.from_audio(audio, features='posteriorgram')
    with pytest.raises(ValueError):
        harmonics.from_audio(audio, decoder='argmax')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harmonics.from_audio(audio)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harmonics.peak_pick(torch.zeros(4, 8), torch.arange(8.))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        viterbi.from_probabilities(torch.full((1, 2, 3), 1 / 3))
    for feature in ('text', 'speaker'):
        with pytest.raises(ValueError, match='out of scope'):
            promonet_amd.preprocess.from_audio(
                audio, gpu=0, features=['loudness', feature])


def test_library_checks_its_arguments_without_a_gpu():
    for name in ('pm_viterbi_workspace', 'pm_viterbi',
                 'pm_harmonics_highpass', 'pm_harmonics_stft',
                 'pm_harmonics_observation', 'pm_harmonics_peaks'):
        assert name in _lib.SIGNATURES
    library = _lib.lib()
    assert library.pm_viterbi_workspace(32, 861, 2039) == \
        -(-32 * 861 * 2039 * 2 // 256) * 256
    assert library.pm_viterbi_workspace(1, 1, 40000) == 0
    fake = ctypes.c_void_p(256)

    def decode(states, band_floats=4):
        return library.pm_viterbi(
            fake, None, fake, band_floats, fake, fake, fake, 1, 1, states,
            fake, 1 << 30, None)

    assert decode(40000) == _lib.PM_EINVAL
    assert 'int16' in library.pm_last_error().decode()
    assert decode(32768) == _lib.PM_EINVAL
    assert decode(20000) == _lib.PM_EINVAL
    assert 'LDS' in library.pm_last_error().decode()
    assert decode(0) == _lib.PM_EINVAL
    assert decode(8, band_floats=6) == _lib.PM_EINVAL
    assert library.pm_viterbi(
        fake, None, fake, 4, fake, fake, fake, 1, 1, 8, fake, 0,
        None) == _lib.PM_ENOMEM
    assert library.pm_harmonics_stft(
        fake, fake, fake, fake, fake, 1, 4096, 1, 2039, 11, 256,
        None) == _lib.PM_EINVAL
    assert library.pm_harmonics_highpass(
        fake, None, fake, 1, 100, 50, 100, 1., 0., 0., 0., 0.,
        None) == _lib.PM_EINVAL
    assert library.pm_harmonics_observation(
        fake, None, fake, None, fake, fake, 1, 1, 0, 0., 0.,
        None) == _lib.PM_EINVAL
    assert library.pm_harmonics_peaks(
        fake, fake, None, fake, 1, 1, 8, -1, None) == _lib.PM_EINVAL
    with pytest.raises(ValueError, match='too short'):
        harmonics.magnitude(torch.zeros(1, 1920), [1920], 22050, 50.)

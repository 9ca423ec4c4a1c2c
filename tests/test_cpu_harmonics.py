"""The harmonics oracle (tests/harmonics_oracle.py), the band packing of
promonet_amd.viterbi and the surface of the new modules. No GPU."""
import ctypes
import inspect

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

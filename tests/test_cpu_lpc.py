"""The LPC oracle (tests/lpc_oracle.py), the facts the device path rests on and
the host side of pm_harmonics_lpc. No GPU.

The yardstick of test_gpu_lpc.py is computed here: per gated case, the
distance of the literal float32 recursion (the reference's arithmetic) from
the float64 one. The device is held to 4 x that.
"""
import ctypes
import inspect

import numpy as np
import pytest
import scipy.signal
import torch

import promonet_amd
from promonet_amd import _lib, viterbi
from promonet_amd.preprocess import harmonics

import harmonics_oracle
import lpc_oracle as oracle

# max |log10 |H| (float32 recursion) - log10 |H| (float64 recursion)| and the
# same for the coefficients, over the 8 frames of each case: computed with
# lpc_oracle.features on the CPU. test_gpu_lpc.py gates at 4 x these.
YARDSTICK = {
    'white': (5.35e-8, 3.89e-8),
    'three resonances, 40 dB floor': (2.73e-5, 3.04e-5),
    'two wide resonances': (1.30e-4, 1.75e-4),
    'four resonances, 40 dB floor': (1.30e-4, 9.66e-5),
}


def autocovariance(a, lags, length=1 << 16):
    """gamma_0 .. gamma_{lags - 1} of unit-variance white noise through
    1 / A(z), from its impulse response"""
    impulse = scipy.signal.lfilter([1.], a, np.eye(1, length)[0])
    return np.array([impulse[:length - k] @ impulse[k:] for k in range(lags)])


@pytest.mark.parametrize('centres,bandwidths', [
    ((2000.,), (300.,)), ((1200., 4000.), (250., 400.))])
def test_burg_recovers_an_autoregressive_process(centres, bandwidths):
    """Order = model order, one long float64 frame. The estimate of an
    AR(p) process from N samples is asymptotically normal about the truth
    with covariance sigma^2 Gamma_p^-1 / N (Gamma_p the p x p autocovariance
    matrix; sigma = 1 here): every coefficient within 5 standard deviations,
    a bound a correct estimator misses once in a million seeds."""
    a = oracle.resonator(centres, bandwidths)
    order = len(a) - 1
    assert order == 2 * len(centres)
    count = 1 << 15
    y = oracle.autoregressive(a, count, seed=order)
    got = oracle.burg(y, order)
    gamma = autocovariance(a, order)
    matrix = gamma[np.abs(np.arange(order)[:, None] - np.arange(order)[None])]
    deviation = np.sqrt(np.diag(np.linalg.inv(matrix)) / count)
    assert got[0] == 1.
    error = np.abs(got[1:] - a[1:])
    print(f'AR({order}): error / standard deviation {error / deviation}')
    assert (error <= 5 * deviation).all()
    assert (deviation < .02).all()
    # the direct sum changes nothing at float64
    np.testing.assert_allclose(
        oracle.burg(y, order, direct=True), got, rtol=0, atol=1e-12)


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_the_denominator_recursion_is_the_direct_sum(name):
    """The Burg identity: den <- (1 - r^2) den - b'[-1]^2 - f'[0]^2 equals
    sum(f^2 + b^2) over the shortened vectors"""
    frame = oracle.frames(oracle.case(name))[3]
    history = []
    oracle.burg(frame, oracle.ORDER, history=history)
    assert len(history) == oracle.ORDER
    worst = max(abs(used - direct) / direct for used, direct in history)
    print(f'{name}: recursion vs direct sum, relative {worst:.2e}')
    assert worst <= 1e-12


def test_a_silent_frame_is_exactly_zero():
    for dtype in (np.float64, np.float32):
        a = oracle.burg(np.zeros(1024), oracle.ORDER, dtype)
        assert a.tolist() == [1.] + [0.] * oracle.ORDER
    result, coefficients = oracle.features(np.zeros(2048, np.float32))
    assert result.shape == (8, 512) and (result == 0).all()
    assert (coefficients[:, 0] == 1).all() and (coefficients[:, 1:] == 0).all()


def test_the_response_is_freqz():
    generator = np.random.RandomState(0)
    for order in (1, 2, 24):
        a = np.concatenate([[1.], .2 * generator.randn(order)])
        _, h = scipy.signal.freqz([1], a, worN=512)
        np.testing.assert_allclose(
            oracle.response(a), np.abs(h), rtol=1e-12, atol=0)
    # a resonator peaks at its centre frequency, on freqz's grid
    a = oracle.resonator((2000.,), (50.,))
    peak = int(np.argmax(oracle.response(a)))
    assert abs(peak * oracle.SAMPLE_RATE / 1024 - 2000.) < 22.


@pytest.mark.parametrize('samples', [255, 256, 1024, 1100, 4096])
def test_frame_count(samples):
    padded = torch.nn.functional.pad(
        torch.zeros(1, samples), (oracle.PADDING, oracle.PADDING))
    want = 0
    if padded.shape[-1] >= oracle.WINDOW_SIZE:
        want = torch.nn.functional.unfold(
            padded[:, None, None], kernel_size=(1, oracle.WINDOW_SIZE),
            stride=(1, oracle.HOPSIZE)).shape[-1]
    assert oracle.frame_count(samples) == want
    assert oracle.frame_count(samples) == max(
        0, (samples + 768 - 1024) // 256 + 1)
    assert harmonics.lpc_frames(samples) == want
    assert harmonics.lpc_frames(torch.tensor([samples])).tolist() == [want]
    assert len(oracle.frames(np.zeros(samples, np.float32))) == want


def test_frequencies_are_the_references():
    frequencies = oracle.frequencies()
    assert frequencies.shape == (512,) and frequencies.dtype == torch.float32
    assert frequencies[0] == 0.
    assert abs(float(frequencies[1]) - 22050 / 1023) < 1e-4
    assert oracle.ORDER == 24


def test_the_decoder_model_is_nan_with_bin_0_and_packs_without():
    frequencies = oracle.frequencies()
    transition, initial = harmonics_oracle.decoder_model(frequencies)
    assert transition[:, 0].isnan().all()
    assert not transition[:, 1:].isnan().any()
    transition, initial = harmonics_oracle.decoder_model(frequencies[1:])
    assert transition.shape == (511, 511)
    assert transition.isfinite().all() and initial.isfinite().all()
    packed = viterbi.Transition(transition)
    assert int(packed.table[1].max()) == 167
    with np.errstate(divide='ignore'):
        assert torch.equal(packed.dense(), torch.log(transition))


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_yardstick(name):
    """The constants test_gpu_lpc.py gates with are this oracle's: float32
    recursion against float64, by a fixed summation tree: the same bits
    on every host up to its hamming_window, for which 10 % is left"""
    audio = oracle.case(name)
    assert len(audio) == 2048 and audio.dtype == np.float32
    exact, exact_coefficients = oracle.features(audio)
    single, single_coefficients = oracle.features(audio, np.float32)
    measured = (np.abs(single - exact).max(),
                np.abs(single_coefficients - exact_coefficients).max())
    print(f'{name}: float32 recursion vs float64: features '
          f'{measured[0]:.3e}, coefficients {measured[1]:.3e}')
    for value, recorded in zip(measured, YARDSTICK[name]):
        assert .9 * recorded <= value <= 1.1 * recorded
    # the direct sum at float32 is no worse than the recursion
    direct, _ = oracle.features(audio, np.float32, direct=True)
    assert np.abs(direct - exact).max() <= 1.5 * measured[0]


def test_module_surface_and_argument_checks():
    assert 'pm_harmonics_lpc' in _lib.SIGNATURES
    for name in ('from_file', 'from_file_to_file'):
        parameters = inspect.signature(getattr(harmonics, name)).parameters
        assert list(parameters)[-2:] == ['gpu', 'features']
        assert parameters['features'].default == 'stft'
    assert list(inspect.signature(harmonics.lpc_coefficients).parameters)[:5] \
        == ['audio', 'sample_rate', 'lengths', 'gpu', 'return_coefficients']
    assert 'unpinned' in harmonics.lpc_coefficients.__doc__
    assert 'librosa' in harmonics.__doc__
    with pytest.raises(ValueError, match='librosa'):
        harmonics.from_audio(torch.zeros(1, 4096), features='lpc')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harmonics.lpc_coefficients(torch.zeros(1, 4096))
    with pytest.raises(ValueError, match='unknown features'):
        harmonics.from_audio(torch.zeros(1, 4096), features='mfcc')

    library = _lib.lib()
    fake = ctypes.c_void_p(256)

    def launch(rows=1, stride=2048, samples=2048, frames=8, order=24,
               window=fake, table=fake):
        return library.pm_harmonics_lpc(
            fake, None, window, table, fake, None, rows, stride, samples,
            frames, order, None)

    for bad in (dict(order=0), dict(order=33), dict(rows=-1),
                dict(samples=-1), dict(frames=-1), dict(stride=2047),
                dict(window=ctypes.c_void_p(260)),
                dict(table=ctypes.c_void_p(264)), dict(window=None),
                dict(rows=1 << 20, frames=1 << 14),
                dict(rows=1 << 13, frames=(1 << 13) + 1)):
        assert launch(**bad) == _lib.PM_EINVAL, bad
    assert launch(order=0) == _lib.PM_EINVAL
    assert '1 to 32' in library.pm_last_error().decode()
    # nothing to do is not an error, and touches nothing
    assert launch(rows=0) == _lib.PM_OK
    assert launch(frames=0) == _lib.PM_OK

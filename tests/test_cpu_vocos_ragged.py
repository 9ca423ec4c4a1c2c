"""Ragged Vocos without a GPU: host-side argument checking of
`pm_vocos_forward_ragged`, its place in the ctypes table, the validation of
`lengths` in Python and the empty case of the batched file entry."""
import ctypes
import inspect

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.model import vocos

BASELINE = dict(MODEL='vocos', SPECTROGRAM_ONLY=True, AUGMENT_PITCH=False,
                AUGMENT_LOUDNESS=False, VOCOS_LAYERS=8)
RESTORE = dict(MODEL='hifigan', SPECTROGRAM_ONLY=False, AUGMENT_PITCH=True,
               AUGMENT_LOUDNESS=True, VOCOS_LAYERS=6)


@pytest.fixture
def baseline():
    promonet_amd.configure(**BASELINE)
    yield
    promonet_amd.configure(**RESTORE)


def test_signatures_hold_both_entries():
    result, arguments = _lib.SIGNATURES['pm_vocos_ragged_workspace_bytes']
    assert result is ctypes.c_size_t and len(arguments) == 3
    result, arguments = _lib.SIGNATURES['pm_vocos_forward_ragged']
    assert result is ctypes.c_int and len(arguments) == 11
    # one more argument than the uniform entry: lengths
    assert len(arguments) == len(_lib.SIGNATURES['pm_vocos_forward'][1]) + 1


def test_ragged_forward_checks_its_arguments():
    lib = _lib.lib()
    handle = ctypes.c_void_p()
    _lib.check(lib.pm_vocos_create(
        80, 256, 512, 1536, 2, 1024, 256, _lib.PM_BF16, ctypes.byref(handle)))
    try:
        # (1 stands in for a device pointer: nothing is dereferenced before
        # the checks fail)
        assert lib.pm_vocos_forward_ragged(
            handle, 1, None, 1, None, 1, 1, 4, 1, 1 << 30, None) == \
            _lib.PM_EINVAL
        assert b'null' in lib.pm_last_error()
        assert lib.pm_vocos_forward_ragged(
            None, 1, None, 1, 1, 1, 1, 4, 1, 1 << 30, None) == _lib.PM_EINVAL
        # not finalised
        assert lib.pm_vocos_forward_ragged(
            handle, 1, None, 1, 1, 1, 1, 4, 1, 1 << 30, None) == \
            _lib.PM_ESTATE
        assert b'finalize' in lib.pm_last_error()
        for batch, frames in ((2, 10), (1, 1), (32, 861)):
            ragged = lib.pm_vocos_ragged_workspace_bytes(handle, batch, frames)
            uniform = lib.pm_vocos_workspace_bytes(handle, batch, frames)
            assert ragged > 0 and ragged >= uniform
            # the row map and the offsets are all it adds
            assert ragged - uniform <= 16 * batch * frames + 4 * batch + 1024
        assert lib.pm_vocos_ragged_workspace_bytes(handle, 0, 10) == 0
        assert lib.pm_vocos_ragged_workspace_bytes(handle, 2, 0) == 0
        assert lib.pm_vocos_ragged_workspace_bytes(None, 2, 10) == 0
    finally:
        lib.pm_vocos_destroy(handle)


def test_forward_takes_lengths():
    for function in (promonet_amd.model.Vocos.forward,
                     promonet_amd.model.MelGenerator.forward):
        parameter = inspect.signature(function).parameters['lengths']
        assert parameter.default is None


def test_cpu_tensor_with_lengths_raises(baseline):
    model = promonet_amd.model.Vocos(80, 256)
    with pytest.raises(RuntimeError, match='GPU'):
        model(torch.zeros(2, 80, 4), lengths=[4, 2])


def test_lengths_shape_is_checked():
    for lengths in ([4, 2, 1], [4], [[4, 2]], 4,
                    torch.tensor([4, 2, 1]), torch.zeros(2, 1, dtype=torch.int)):
        with pytest.raises(ValueError, match='shape'):
            vocos.check_lengths(lengths, 2, 4)
    with pytest.raises(ValueError, match='integers'):
        vocos.check_lengths([4., 2.], 2, 4)


@pytest.mark.parametrize('lengths', [[0, 4], [4, 5], [-1, 4],
                                     torch.tensor([4, 0]),
                                     torch.tensor([9, 1], dtype=torch.int32)])
def test_host_lengths_are_range_checked(lengths):
    with pytest.raises(ValueError, match=r'\[1, 4\]'):
        vocos.check_lengths(lengths, 2, 4)


def test_valid_lengths_pass():
    for lengths in ([4, 1], (1, 4), torch.tensor([2, 3])):
        got = vocos.check_lengths(lengths, 2, 4)
        assert got.shape == (2,) and got.tolist() == list(lengths)


def test_batched_files_with_nothing_to_do():
    # no device is named and none is touched
    mels = promonet_amd.baseline.mels
    assert mels.from_files_to_files_batched([], []) is None
    assert mels.from_files_to_files_batched([], [], speakers=[], gpu=None,
                                            batch_size=3) is None
    parameters = inspect.signature(mels.from_files_to_files_batched).parameters
    assert list(parameters) == [
        'audio_files', 'output_files', 'speakers', 'spectral_balance_ratio',
        'loudness_ratio', 'checkpoint', 'gpu', 'batch_size']
    assert parameters['batch_size'].default == 32

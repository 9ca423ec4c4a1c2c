"""Vocos without a GPU: the restatement against the real-reference golden,
the drop-in's state-dict layout and configuration, host-side validation of
the engine and the patch of the mel vocoder."""
import ctypes
import types

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
import vocos_oracle as oracle
from conftest import GOLDEN

BASELINE = dict(MODEL='vocos', SPECTROGRAM_ONLY=True, AUGMENT_PITCH=False,
                AUGMENT_LOUDNESS=False, VOCOS_LAYERS=8)
RESTORE = dict(MODEL='hifigan', SPECTROGRAM_ONLY=False, AUGMENT_PITCH=True,
               AUGMENT_LOUDNESS=True, VOCOS_LAYERS=6)


@pytest.fixture
def baseline():
    promonet_amd.configure(**BASELINE)
    yield
    promonet_amd.configure(**RESTORE)


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN / 'vocos.pt', weights_only=False)


def test_restatement_equals_the_reference_golden(golden):
    state = oracle.random_state_vocos(int(golden['seed']))
    table = torch.randn(109, 256, generator=torch.Generator().manual_seed(
        int(golden['speaker_table_seed'])))
    case = 0
    while f'case{case}/mels' in golden:
        g = oracle.global_features(golden[f'case{case}/speakers'], table)
        got = oracle.vocos(golden[f'case{case}/mels'], g, state)
        want = golden[f'case{case}/audio']
        assert got.shape == want.shape
        assert (got - want).abs().max().item() <= 1e-6, case
        case += 1
    assert case >= 4


def test_mel_generator_layout_matches_the_reference(baseline, golden):
    state = promonet_amd.model.MelGenerator().state_dict()
    shapes = {k[len('shape/'):]: tuple(v.tolist())
              for k, v in golden.items() if k.startswith('shape/')}
    assert {k: tuple(v.shape) for k, v in state.items()} == shapes
    assert len(state) == int(golden['num_entries']) == 87
    assert sum(v.numel() for v in state.values()) == \
        int(golden['num_elements']) == 15456003


def test_restatement_state_loads_into_the_drop_in(baseline):
    model = promonet_amd.model.Vocos(80, 256)
    model.load_state_dict(oracle.random_state_vocos(0))
    assert model.head.istft.window.shape == (1024,)


def test_configure_derives_the_baseline_constants(baseline):
    assert promonet_amd.NUM_FEATURES == 80
    assert promonet_amd.GLOBAL_CHANNELS == 256
    assert promonet_amd.VOCOS_LAYERS == 8
    assert promonet_amd.VOCOS_CHANNELS == 512
    assert promonet_amd.VOCOS_POINTWISE_CHANNELS == 1536


def test_reference_defaults():
    assert promonet_amd.config.VOCOS_LAYERS == 6
    assert promonet_amd.config.SPARSE_MELS is False


def test_generator_points_at_mel_generator(baseline):
    with pytest.raises(ValueError, match='MelGenerator'):
        promonet_amd.model.Generator()


def test_vocos_dtypes():
    from promonet_amd.model.vocos import resolve_dtype
    assert resolve_dtype('checkpoint') == 'fp32'
    assert resolve_dtype('bf16') == 'bf16'
    for name in ('f16a2', 'f16x3', 'f16+f16+f16+f16', 'mixed'):
        with pytest.raises(ValueError):
            resolve_dtype(name)


@pytest.mark.parametrize('args', [
    (80, 256, 256, 1536, 8, 1024, 256, _lib.PM_F32),   # channels
    (80, 256, 512, 1000, 8, 1024, 256, _lib.PM_F32),   # hidden
    (81, 256, 512, 1536, 8, 1024, 256, _lib.PM_F32),   # features
    (80, 0, 512, 1536, 8, 1024, 256, _lib.PM_F32),     # global channels
    (80, 256, 512, 1536, -1, 1024, 256, _lib.PM_F32),  # layers
    (80, 256, 512, 1536, 8, 2048, 256, _lib.PM_F32),   # n_fft
    (80, 256, 512, 1536, 8, 1024, 128, _lib.PM_F32),   # hop
    (80, 256, 512, 1536, 8, 1024, 256, _lib.PM_F16A2),  # dtype
])
def test_vocos_create_rejects_bad_configs(args):
    lib = _lib.lib()
    handle = ctypes.c_void_p()
    assert lib.pm_vocos_create(*args, ctypes.byref(handle)) == _lib.PM_EINVAL
    assert not handle.value
    assert lib.pm_last_error()


def test_vocos_create_checks_names_and_order():
    lib = _lib.lib()
    handle = ctypes.c_void_p()
    _lib.check(lib.pm_vocos_create(
        80, 256, 512, 1536, 2, 1024, 256, _lib.PM_BF16, ctypes.byref(handle)))
    try:
        assert lib.pm_vocos_finalize(handle, None) == _lib.PM_ESTATE
        assert b'was not loaded' in lib.pm_last_error()
        shape = _lib.shape_array((3,))
        assert lib.pm_vocos_load_tensor(
            handle, b'no.such.key', 1, shape, 1, None) == _lib.PM_EINVAL
        assert lib.pm_vocos_load_tensor(
            handle, b'conv_pre.bias', 1, shape, 1, None) == _lib.PM_EINVAL
        assert b'shape' in lib.pm_last_error()
        assert lib.pm_vocos_forward(
            handle, 1, None, 1, 1, 1, 4, 1, 1 << 30, None) == _lib.PM_ESTATE
        assert lib.pm_vocos_workspace_bytes(handle, 2, 10) > 0
    finally:
        lib.pm_vocos_destroy(handle)


def test_patch_swaps_the_mel_vocoder_only_where_present():
    def stand_in(with_vocos):
        promonet = types.SimpleNamespace()
        promonet.model = types.SimpleNamespace(
            HiFiGAN=None, FARGAN=None, Generator=None)
        promonet.synthesize = types.SimpleNamespace()
        promonet.preprocess = types.SimpleNamespace(
            spectrogram=types.SimpleNamespace(),
            loudness=types.SimpleNamespace())
        if with_vocos:
            promonet.model.Vocos = promonet.model.MelGenerator = None
            promonet.baseline = types.SimpleNamespace(
                mels=types.SimpleNamespace(**{name: None for name in (
                    'from_audio', 'from_features', 'from_file',
                    'from_file_to_file', 'from_files_to_files',
                    'resample')}))
        return promonet

    patched = promonet_amd.patch(stand_in(True))
    assert patched.model.Vocos is promonet_amd.model.Vocos
    assert patched.model.MelGenerator is promonet_amd.model.MelGenerator
    for name in ('from_audio', 'from_features', 'from_file',
                 'from_file_to_file', 'from_files_to_files', 'resample'):
        assert getattr(patched.baseline.mels, name) is \
            getattr(promonet_amd.baseline.mels, name)
    bare = promonet_amd.patch(stand_in(False))
    assert not hasattr(bare.model, 'Vocos')
    assert not hasattr(bare.model, 'MelGenerator')
    assert not hasattr(bare, 'baseline')

"""The discriminator spectrograms without a GPU: the float64 oracle
(tests/disc_spectrogram_oracle.py) against the reference's own run
(tests/golden/disc_spectrogram.pt), the conditions the GPU tests rely on, the
planted defects their comparison must reject, `patch()` and the size checks.
"""
import types
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.model import discriminator

import disc_spectrogram_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'disc_spectrogram.pt')


def close(got, want):
    return (got - want).abs().max() <= 1e-12 * want.abs().max()


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_equals_the_reference(golden, name):
    want, kept = oracle.truth(name), golden[name]
    assert torch.equal(want['x'][:, :8], kept['head'])
    assert list(want['out'].shape) == kept['shape']
    frames = kept['shape'][2 if oracle.CASES[name][0] == 'CMB' else -1]
    assert frames == oracle.FRAMES[name]
    assert kept['out'].dtype == kept['gradient'].dtype == torch.float64
    assert close(
        want['out'].flatten()[::golden['output_stride']], kept['out'])
    assert close(
        want['gradient'].flatten()[::golden['gradient_stride']],
        kept['gradient'])


def test_the_band_edges_are_the_reference_s(golden):
    assert [tuple(e) for e in golden['edges']] == list(oracle.DEFAULT_EDGES)
    assert discriminator.band_edges() == list(oracle.DEFAULT_EDGES)
    widths = [high - low for low, high in oracle.DEFAULT_EDGES]
    assert widths == [51, 77, 128, 128, 129]


@pytest.mark.parametrize('name', NAMES)
def test_the_inputs_meet_what_the_gpu_tests_rely_on(name):
    kind, sizes, _ = oracle.CASES[name]
    want = oracle.truth(name)
    share = want['fragile'].double().mean().item()
    assert share <= 1e-3, share
    assert not want['upstream'][want['fragile']].any()
    if kind != 'DB':
        return
    X = oracle.transform(oracle.flat(want['x']), kind, sizes).abs()
    x_db = 20. * torch.log10(X.clamp(min=oracle.AMIN))
    floor = x_db.max() - oracle.TOP_DB
    assert int((x_db == x_db.max()).sum()) == 1       # a unique maximum
    assert not (x_db == floor).any()                  # no element at the floor
    assert not (x_db[0] < floor).any()
    floored = (x_db[1] < floor).double().mean().item()
    assert .2 <= floored <= .9, floored
    # the floored elements show the floor, and it is row 0 that sets it
    assert torch.equal(want['out'] == floor, x_db < floor)
    assert x_db[0].max() == x_db.max()


@pytest.mark.parametrize('name', NAMES)
def test_the_gates_come_from_the_reference_arithmetic_in_fp32(name):
    """K = 4 x the largest recorded figure of the family; the fp32 torch
    arithmetic itself, run here, stays inside its gates"""
    forward, gradient = oracle.fp32_figures(name)
    print(f'{name}: fp32 torch forward {forward:.3f}, gradient '
          f'{gradient:.3f} (recorded {oracle.FP32_RECORDED[name]})')
    assert forward < oracle.gate(name, 'forward')
    assert gradient < oracle.gate(name, 'gradient')
    for i, direction in enumerate(('forward', 'gradient')):
        assert oracle.gate(name, direction) >= \
            4. * oracle.FP32_RECORDED[name][i]
        assert oracle.gate(name, direction) == 4. * max(
            oracle.FP32_RECORDED[other][i] for other in NAMES
            if oracle.family(other) == oracle.family(name))


###############################################################################
# Planted defects: the comparison of the GPU tests (shapes, the forward figure
# on the non-fragile elements, the gradient figure) rejects each of them in
# every case it can touch
###############################################################################

APPLIES = {
    'pad_off_by_one': NAMES,
    'pad_half': ['R-512', 'R-1024', 'R-2048', 'CMB'],
    'window_left': ['R-512', 'R-1024', 'R-2048'],
    'window_hann': ['R-512', 'R-1024', 'R-2048', 'CMB'],
    'row_maximum': ['DB-64', 'DB-256', 'DB-2048'],
    'floor_gradient_dropped': ['DB-64', 'DB-256', 'DB-2048'],
    'band_edge': ['CMB'],
    'swapped_axes': ['CMB'],
    'right_margin_not_folded': NAMES,
}


def accepted(name, defect):
    """Would the GPU tests pass an implementation with this defect?"""
    kind, sizes, _ = oracle.CASES[name]
    want = oracle.truth(name)
    if kind == 'CMB':
        bands = oracle.multiband(want['x'], sizes[0], sizes[1], defect=defect)
        right = oracle.multiband(want['x'], sizes[0], sizes[1])
        if [b.shape for b in bands] != [b.shape for b in right]:
            return False
    out = oracle.output(kind, want['x'], sizes, defect)
    if out.shape != want['out'].shape:
        return False
    if not oracle.figure_forward(name, out) < oracle.gate(name, 'forward'):
        return False
    gradient = oracle.gradient(kind, want['x'], sizes, want['upstream'],
                               defect)
    return oracle.figure_gradient(name, gradient) < \
        oracle.gate(name, 'gradient')


def test_the_defects_are_all_listed():
    assert set(APPLIES) == set(oracle.DEFECTS)


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_itself_is_accepted(name):
    assert accepted(name, None)


@pytest.mark.parametrize(
    'defect,name',
    [(defect, name) for defect in oracle.DEFECTS for name in APPLIES[defect]])
def test_a_planted_defect_is_rejected(defect, name):
    assert not accepted(name, defect)


###############################################################################
# patch()
###############################################################################


def stand_in(with_discriminator=True):
    calls = []

    def method(label):
        def spectrogram(self, x):
            calls.append(label)
            return label
        return spectrogram

    promonet = types.SimpleNamespace(
        model=types.SimpleNamespace(HiFiGAN=None, FARGAN=None, Generator=None),
        synthesize=types.SimpleNamespace(),
        preprocess=types.SimpleNamespace(
            spectrogram=types.SimpleNamespace(),
            loudness=types.SimpleNamespace()))
    if with_discriminator:
        promonet.model.discriminator = types.SimpleNamespace(**{
            name: type(name, (), {'spectrogram': method(name)})
            for name in ('DiscriminatorR', 'DiscriminatorCMB',
                         'SpecDiscriminatorBase')})
        promonet.model.discriminator.DiscriminatorMagFree = type(
            'DiscriminatorMagFree',
            (promonet.model.discriminator.SpecDiscriminatorBase,), {})
    return promonet, calls


def test_patch_swaps_the_three_methods_and_keeps_the_originals():
    promonet, calls = stand_in()
    module = promonet.model.discriminator
    before = {name: getattr(module, name).spectrogram
              for name in ('DiscriminatorR', 'DiscriminatorCMB',
                           'SpecDiscriminatorBase')}
    promonet_amd.patch(promonet)
    for name, original in before.items():
        method = getattr(module, name).spectrogram
        assert method is not original and method.original is original
        # a CPU tensor goes to the original method
        assert getattr(module, name)().spectrogram(torch.zeros(1, 1, 8)) == name
    # the subclass the FARGAN configurations build inherits the wrapper
    assert module.DiscriminatorMagFree().spectrogram(
        torch.zeros(1, 1, 8)) == 'SpecDiscriminatorBase'
    assert calls == ['DiscriminatorR', 'DiscriminatorCMB',
                     'SpecDiscriminatorBase', 'SpecDiscriminatorBase']
    # patching twice wraps once
    promonet_amd.patch(promonet)
    assert module.DiscriminatorR.spectrogram.original is \
        before['DiscriminatorR']


def test_patch_leaves_a_package_without_discriminators_alone():
    promonet, _ = stand_in(with_discriminator=False)
    promonet_amd.patch(promonet)
    assert not hasattr(promonet.model, 'discriminator')


###############################################################################
# Sizes: ValueError from Python, PM_EINVAL from the ABI, no device needed
###############################################################################

BAD = [
    ('resolution', (2, 4000), (1000, 100, 1000)),    # not 2^a or 5 2^a
    ('resolution', (2, 4000), (32, 8, 32)),          # below 64
    ('resolution', (2, 4000), (4096, 1024, 4096)),   # above 2560
    ('resolution', (2, 4000), (512, 0, 240)),        # hop < 1
    ('resolution', (2, 4000), (512, 513, 240)),      # hop > N
    ('resolution', (2, 4000), (512, 50, 600)),       # win > N
    ('resolution', (2, 231), (512, 50, 240)),        # T <= pad
    ('decibel', (2, 1024), (2048, 512, 2048)),       # T <= pad = N / 2
    ('resolution', (2, 40), (64, 64, 64)),           # less than one frame
    ('resolution', (2, 4000), (512, 50)),            # no resolution
    ('resolution', (2, 2, 4000), (512, 50, 240)),    # not (B, 1, T)
]


@pytest.mark.parametrize('which,shape,sizes', BAD)
def test_bad_sizes_raise_before_any_device_work(which, shape, sizes):
    function = getattr(discriminator, f'spectrogram_{which}')
    with pytest.raises(ValueError):
        function(torch.zeros(shape), sizes)


def test_multiband_refuses_a_band_outside_the_bins():
    with pytest.raises(ValueError):
        discriminator.spectrogram_multiband(
            torch.zeros(2, 2300), bands=((0., 1.1),))
    with pytest.raises(ValueError):
        discriminator.spectrogram_multiband(torch.zeros(2, 384))


def test_good_sizes_on_a_cpu_tensor_say_that_there_is_no_fallback():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.spectrogram_resolution(
            torch.zeros(2, 700), (512, 50, 240))


ABI_BAD = [
    # mode, batch, samples, fft_size, hop_size, win_length, pad
    (3, 2, 4000, 512, 50, 240, 231),
    (0, 0, 4000, 512, 50, 240, 231),
    (0, 2, 4000, 1000, 100, 1000, 450),
    (0, 2, 4000, 32, 8, 32, 12),
    (0, 2, 4000, 5120, 1024, 4096, 2048),
    (0, 2, 4000, 512, 0, 240, 231),
    (0, 2, 4000, 512, 513, 240, 0),
    (0, 2, 4000, 512, 50, 600, 231),
    (0, 2, 4000, 512, 50, 240, -1),
    (0, 2, 231, 512, 50, 240, 231),
    (2, 2, 1024, 2048, 512, 2048, 1024),
    (0, 2, 40, 64, 64, 64, 0),
]


@pytest.mark.parametrize('arguments', ABI_BAD)
def test_the_abi_refuses_bad_sizes_on_the_host(arguments):
    library = _lib.lib()
    mode, *rest = arguments
    assert library.pm_disc_spec_workspace_bytes(mode, *rest, 0) == 0
    assert library.pm_disc_spec_workspace_bytes(mode, *rest, 1) == 0
    # (the pointers are never read: the sizes are refused first)
    code = library.pm_disc_spec_forward(
        mode, 256, 256, 256, 256, 256, *rest, 256, 1 << 30, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_disc_spec_forward' in library.pm_last_error()
    code = library.pm_disc_spec_backward(
        mode, 256, 256, 256, 256, 256, 256, None, 256, 0, *rest, 256,
        1 << 30, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_disc_spec_backward' in library.pm_last_error()


def test_the_abi_refuses_null_pointers_and_a_small_workspace():
    library = _lib.lib()
    sizes = (2, 1000, 64, 16, 64, 32)
    need = library.pm_disc_spec_workspace_bytes(2, *sizes, 1)
    assert need >= 256 and need % 256 == 0
    assert library.pm_disc_spec_workspace_bytes(0, *sizes, 0) == 256
    code = library.pm_disc_spec_forward(
        2, 256, 256, 256, 256, None, *sizes, 256, 1 << 30, None)
    assert code == _lib.PM_EINVAL
    code = library.pm_disc_spec_backward(
        2, 256, 256, 256, 256, 256, 256, None, 256, 0, *sizes, 256,
        need - 1, None)
    assert code == _lib.PM_ENOMEM

"""The conv stacks of the complex multi-band and the multi-resolution
discriminators without a GPU: the float64 oracle (tests/dconv_oracle.py)
against torch's conv2d and against the reference's own run
(tests/golden/dconv.pt), the state_dicts, the conditions the GPU tests rely
on, the planted defects their comparison must reject, the size checks and
`patch()`.
"""
import math
import types
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.model import discriminator

import conv_checks
import dconv_oracle as oracle
from conv_checks import close

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
ALL_NAMES = list(oracle.ALL_CASES)
STACKS = ('cmb', 'r')


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'dconv.pt')


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('name', ALL_NAMES)
def test_the_layer_oracle_equals_conv2d_in_float64(name):
    _, _, _, stride, _, _, slope = oracle.ALL_CASES[name]
    want = oracle.truth(name)
    _, y, gradients = oracle.reference_fp32(
        want['x'], want['weight'], want['bias'], stride, slope,
        torch.float64, want['upstream'])
    assert want['forward'].shape == y.shape
    assert close(want['forward'], y)
    for quantity, theirs in zip(oracle.QUANTITIES[1:], gradients):
        assert want[quantity].shape == theirs.shape
        assert close(want[quantity], theirs), quantity


def test_the_forms_are_the_module_s():
    assert oracle.FORMS == discriminator.BAND_FORMS
    assert {case[:4] for case in oracle.CASES.values()} == set(oracle.FORMS)
    assert {case[6] for case in oracle.CASES.values()} == {.1, .2, 1.}


def test_the_parameters_are_exact_in_fp32_and_keep_g_away_from_the_norm():
    for name in STACKS:
        for key, value in oracle.parameters(name).items():
            assert value.dtype == torch.float32
            scaled = value.double() * 2 ** 14
            assert torch.equal(scaled, scaled.round())
            if key.endswith('weight_g'):
                assert value.min() >= .5
                norm = oracle.parameters(name)[
                    key[:-1] + 'v'].double().flatten(1).norm(dim=1)
                assert ((value.flatten().double() - norm).abs() > .1).all()


def stack_of(golden, name, defect=None):
    kept = golden['stacks'][name]
    x = kept['x']
    assert torch.equal(x, oracle.stack_input(name))
    inputs = [x[..., low:high] for low, high in oracle.CMB_EDGES] \
        if name == 'cmb' else [x]
    return kept, oracle.stack(name, inputs, oracle.parameters(name), defect)


golden_coefficients = oracle.golden_coefficients
stack_figures = oracle.stack_figures


@pytest.mark.parametrize('name', STACKS)
def test_the_stack_oracle_equals_the_reference(golden, name):
    kept, (logits, maps, saved) = stack_of(golden, name)
    assert kept['logits'].dtype == torch.float64
    assert [list(m.shape) for m in maps] == kept['map_shapes']
    assert len(maps) == (26 if name == 'cmb' else 6)
    grad_inputs, gradients, _ = oracle.stack_backward(
        saved, oracle.parameters(name), golden_coefficients(golden, name))
    for label, _, value in stack_figures(
            golden, name, logits, maps[:-1], torch.cat(grad_inputs, dim=-1),
            gradients):
        assert value <= 1e-12, (label, value)


@pytest.mark.parametrize('name', STACKS)
def test_the_mended_functional_carries_nothing_to_a_fragile_element(
        golden, name):
    _, (_, maps, saved) = stack_of(golden, name)
    mended = golden['stacks'][name]['mended']
    _, _, again = oracle.stack_backward(
        saved, oracle.parameters(name),
        oracle.coefficients(name, [m.shape for m in maps]), mend=True)
    plain = oracle.coefficients(name, [m.shape for m in maps])
    for mine, theirs, before in zip(
            again, golden_coefficients(golden, name), plain):
        # the same elements; the values to an ulp of fp32 (they are float64
        # sums rounded once, whose last bit may depend on the machine)
        assert torch.equal(mine != before, theirs != before)
        assert torch.allclose(mine, theirs, rtol=2. ** -22, atol=0.)
    assert 0 < len(mended[0]) < 200


###############################################################################
# The state_dicts
###############################################################################


@pytest.mark.parametrize('name', STACKS)
def test_the_module_has_the_reference_s_keys_and_shapes(golden, name):
    module = discriminator.DiscriminatorCMB() if name == 'cmb' \
        else discriminator.DiscriminatorR(golden['resolution'])
    state = module.state_dict()
    assert list(state) == golden['keys'][name]
    assert [list(v.shape) for v in state.values()] == golden['shapes'][name]
    assert list(oracle.shapes(name)) == golden['keys'][name]
    parameters = oracle.parameters(name)
    module.load_state_dict(parameters)
    key = golden['keys'][name][-4]
    assert torch.equal(module.state_dict()[key], parameters[key])
    if name == 'cmb':
        assert discriminator.band_edges(module.bands) == \
            [tuple(band) for band in golden['bands']]


###############################################################################
# What the GPU tests rely on
###############################################################################


@pytest.mark.parametrize('name', ALL_NAMES)
def test_the_fragile_share_is_small(name):
    conv_checks.the_fragile_share_is_small(oracle, name)


def test_the_walked_case_has_more_tiles_than_compute_units():
    _, _, _, stride, height, width, _ = oracle.ALL_CASES['walked']
    rows, columns = oracle.CONSTANTS['DC_ROWS'], oracle.CONSTANTS['DC_COLS']
    out_width = (width - 1) // stride + 1
    assert oracle.BATCH * math.ceil(height / rows) * \
        math.ceil(out_width / columns) > 256
    assert oracle.BATCH * math.ceil(height / rows) * \
        math.ceil(width / (columns * stride)) > 256


def test_the_large_case_reaches_past_one_workgroup_and_one_partial():
    channels, out_channels, kernel_width, stride, height, width, _ = \
        oracle.CASES['large']
    rows, columns = oracle.CONSTANTS['DC_ROWS'], oracle.CONSTANTS['DC_COLS']
    out_width = (width - 1) // stride + 1
    tiles = oracle.BATCH * math.ceil(height / rows) * \
        math.ceil(out_width / columns)
    assert tiles >= 2 * oracle.CONSTANTS['DC_GW_MIN_TILES']
    # a last tile that is partly empty, in both directions
    assert height % rows and out_width % columns
    # and the partials of the workspace say so
    library = _lib.lib()
    sizes = (channels, out_channels, height, width, kernel_width, stride)
    need = library.pm_dconv_workspace_bytes(oracle.BATCH, *sizes)
    one = library.pm_dconv_workspace_bytes(1, channels, out_channels, 4, 16,
                                           kernel_width, stride)
    assert one >= 4 * (32 * 32 * 27 + 32) and need >= 2 * one - 256


@pytest.mark.parametrize('name', NAMES)
def test_the_gates_come_from_the_reference_arithmetic_in_fp32(name):
    conv_checks.the_gates_come_from_the_reference_arithmetic_in_fp32(
        oracle, name)


@pytest.mark.parametrize('shape', oracle.WEIGHT_NORM_SHAPES)
def test_the_weight_norm_gates_come_from_torch_in_fp32(shape):
    conv_checks.the_weight_norm_gates_come_from_torch_in_fp32(oracle, shape)


###############################################################################
# Planted defects: the comparison of the GPU tests (the shapes and the four
# figures against the gates) rejects each of them in every case it can touch
###############################################################################

STRIDED = [n for n in NAMES if oracle.CASES[n][3] == 2]
SLOPED = [n for n in NAMES if oracle.CASES[n][6] != 1.]
APPLIES = {
    'stride_on_height': [n for n in STRIDED if n != 'one-row'],
    'padding_swapped': [n for n in NAMES if oracle.CASES[n][2] == 9],
    'taps_flipped': NAMES,
    'taps_transposed': [n for n in NAMES if oracle.CASES[n][2] == 3],
    'width_rounded_up': [n for n in STRIDED if not oracle.CASES[n][5] % 2],
    'slope_on_positive': SLOPED,
    'slope_left_out_of_gz': SLOPED,
    'mask_from_input': SLOPED,
    'gx_odd_taps_dropped': NAMES,
    'gw_padded_columns_dropped': NAMES,
}


def accepted(name, defect):
    """Would the GPU tests pass an implementation with this defect?"""
    _, _, _, stride, _, _, slope = oracle.CASES[name]
    return conv_checks.accepted(
        oracle, name,
        lambda *inputs: oracle.layer(*inputs, stride, slope, defect),
        lambda *inputs: oracle.layer_backward(*inputs, stride, slope, defect))


def test_the_defects_are_all_listed():
    assert set(APPLIES) == set(oracle.DEFECTS)
    assert all(APPLIES.values())


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_itself_is_accepted(name):
    assert accepted(name, None)


@pytest.mark.parametrize(
    'defect,name',
    [(defect, name) for defect in APPLIES for name in APPLIES[defect]])
def test_a_planted_defect_is_rejected(defect, name):
    assert not accepted(name, defect)


def stack_accepted(golden, name, defect):
    kept, (logits, maps, saved) = stack_of(golden, name, defect)
    grad_inputs, gradients, _ = oracle.stack_backward(
        saved, oracle.parameters(name), golden_coefficients(golden, name))
    return all(value < oracle.gate(quantity) for _, quantity, value in
               stack_figures(golden, name, logits, maps[:-1],
                             torch.cat(grad_inputs, dim=-1), gradients))


@pytest.mark.parametrize('name', STACKS)
def test_the_stack_oracle_itself_is_accepted(golden, name):
    assert stack_accepted(golden, name, None)


@pytest.mark.parametrize('defect,name', [
    ('bands_wrong_order', 'cmb'), ('activation_after_post', 'cmb'),
    ('activation_after_post', 'r'), ('maps_before_activation', 'cmb'),
    ('maps_before_activation', 'r')])
def test_a_planted_stack_defect_is_rejected(golden, defect, name):
    assert defect in oracle.STACK_DEFECTS
    assert not stack_accepted(golden, name, defect)


###############################################################################
# Sizes: ValueError from Python, PM_EINVAL from the ABI, no device needed
###############################################################################


def arguments(channels=32, out_channels=32, kernel_width=9, height=5,
              width=9):
    return (torch.zeros(2, channels, height, width),
            torch.zeros(out_channels, channels, 3, kernel_width),
            torch.zeros(out_channels))


BAD = [
    (lambda x, w, b: (x[0], w, b), {'stride': 2}),                # not 4-D
    (lambda x, w, b: (x[:, :16], w[:, :16], b), {'stride': 2}),   # C = 16
    (lambda x, w, b: (x, w[:16], b[:16]), {'stride': 2}),         # O = 16
    (lambda x, w, b: (x[:, :1], w, b), {'stride': 2}),            # C of x
    (lambda x, w, b: (x, w[..., :5], b), {'stride': 2}),          # kw = 5
    (lambda x, w, b: (x, w[:, :, :2], b), {'stride': 2}),         # kh = 2
    (lambda x, w, b: (x, w, b[:1]), {'stride': 2}),               # bias
    (lambda x, w, b: (x[:, :, :0], w, b), {'stride': 2}),         # empty
    (lambda x, w, b: (x.long(), w, b), {'stride': 2}),            # not float
    (lambda x, w, b: (x, w, b), {'stride': 1}),                   # (32,32,9,1)
    (lambda x, w, b: (x, w[..., :3], b), {'stride': 2}),          # (32,32,3,2)
    (lambda x, w, b: (x, w, b), {'stride': (2, 1)}),              # on H
    (lambda x, w, b: (x, w, b), {'stride': 2, 'slope': 0.}),
    (lambda x, w, b: (x, w, b), {'stride': 2, 'slope': 1.5}),
    (lambda x, w, b: (x, w, b), {'stride': 2, 'slope': -.1}),
    (lambda x, w, b: (x, w, b), {'stride': 2, 'slope': float('nan')}),
    (lambda x, w, b: (x, w, b), {'stride': 2, 'slope': float('inf')}),
    (lambda x, w, b: (x, w, b), {'stride': 2, 'slope': 'leaky'}),
]


@pytest.mark.parametrize('change,keywords', BAD)
def test_bad_arguments_raise_before_any_device_work(change, keywords):
    with pytest.raises(ValueError):
        discriminator.band_conv(*change(*arguments()), **keywords)


def test_one_channel_on_both_sides_is_refused():
    with pytest.raises(ValueError):
        discriminator.band_conv(*arguments(1, 1, 3))


@pytest.mark.parametrize('form', oracle.FORMS)
def test_good_sizes_on_a_cpu_tensor_say_that_there_is_no_fallback(form):
    channels, out_channels, kernel_width, stride = form
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.band_conv(
            *arguments(channels, out_channels, kernel_width), stride=stride,
            slope=.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.band_conv(
            *arguments(channels, out_channels, kernel_width),
            stride=(1, stride))


GOOD_SIZES = (2, 32, 32, 5, 9, 9, 2)
ABI_BAD = [
    # batch, channels, out_channels, height, width, kernel_width, stride
    ((2, 16, 32, 5, 9, 9, 2), .1),
    ((2, 32, 16, 5, 9, 9, 2), .1),
    ((2, 1, 1, 5, 9, 3, 1), .1),
    ((2, 32, 32, 5, 9, 9, 1), .1),
    ((2, 32, 32, 5, 9, 3, 2), .1),
    ((2, 1, 32, 5, 9, 9, 2), .1),
    ((2, 1, 32, 5, 9, 3, 1), .1),
    ((2, 32, 1, 5, 9, 9, 1), .1),
    ((2, 32, 32, 5, 9, 5, 2), .1),
    ((2, 32, 32, 5, 9, 9, 0), .1),
    ((0, 32, 32, 5, 9, 9, 2), .1),
    ((2, 32, 32, 0, 9, 9, 2), .1),
    ((2, 32, 32, 5, 0, 9, 2), .1),
    ((1 << 20, 32, 32, 1 << 10, 1 << 10, 9, 2), .1),    # 2^40 pixels
    ((1 << 11, 32, 32, 1 << 10, 1 << 10, 9, 2), .1),    # 2^31 input pixels
    (GOOD_SIZES, 0.),
    (GOOD_SIZES, -.5),
    (GOOD_SIZES, 1.0001),
    (GOOD_SIZES, float('nan')),
    (GOOD_SIZES, float('inf')),
]


@pytest.mark.parametrize('sizes,slope', ABI_BAD)
def test_the_abi_refuses_bad_sizes_on_the_host(sizes, slope):
    library = _lib.lib()
    if sizes != GOOD_SIZES:
        assert library.pm_dconv_workspace_bytes(*sizes) == 0
    # (the pointers are never read: the sizes are refused first)
    code = library.pm_dconv_forward(256, 256, 256, 256, *sizes, slope, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_dconv_forward' in library.pm_last_error()
    code = library.pm_dconv_backward(
        256, 256, 256, 256, 256, 256, 256, *sizes, slope, 256, 1 << 40, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_dconv_backward' in library.pm_last_error()


@pytest.mark.parametrize('form', oracle.FORMS)
def test_the_abi_refuses_null_pointers_and_a_small_workspace(form):
    library = _lib.lib()
    channels, out_channels, kernel_width, stride = form
    sizes = (2, channels, out_channels, 5, 9, kernel_width, stride)
    need = library.pm_dconv_workspace_bytes(*sizes)
    assert need >= 4 * (channels * out_channels * 3 * kernel_width +
                        out_channels) and need % 256 == 0
    for null in range(4):
        pointers = [256] * 4
        pointers[null] = None
        code = library.pm_dconv_forward(*pointers, *sizes, .1, None)
        assert code == _lib.PM_EINVAL
        assert b'pm_dconv_forward' in library.pm_last_error()
    for null in (0, 1, 2, 3, 5, 6):
        pointers = [256] * 7
        pointers[null] = None
        code = library.pm_dconv_backward(
            *pointers, *sizes, .1, 256, need, None)
        assert code == _lib.PM_EINVAL
        assert b'pm_dconv_backward' in library.pm_last_error()
    code = library.pm_dconv_backward(
        *[256] * 7, *sizes, .1, None, need, None)
    assert code == _lib.PM_EINVAL
    code = library.pm_dconv_backward(
        *[256] * 7, *sizes, .1, 256, need - 1, None)
    assert code == _lib.PM_ENOMEM
    assert b'pm_dconv_backward' in library.pm_last_error()


def test_the_workspace_stays_modest_at_any_size():
    library = _lib.lib()
    largest = library.pm_dconv_workspace_bytes(
        1 << 10, 32, 32, 1 << 10, 1 << 10, 9, 2)
    assert 0 < largest <= oracle.CONSTANTS['DC_GW_MAX_PARTS'] * \
        (4 * (32 * 32 * 27 + 32) + 256)
    assert largest < 32 << 20


###############################################################################
# patch()
###############################################################################


def stand_in(with_forward=True):
    members = {'spectrogram': lambda self, x: 'spectrogram'}
    if with_forward:
        members['forward'] = lambda self, x: 'forward'
    promonet = types.SimpleNamespace(
        model=types.SimpleNamespace(HiFiGAN=None, FARGAN=None, Generator=None),
        synthesize=types.SimpleNamespace(),
        preprocess=types.SimpleNamespace(
            spectrogram=types.SimpleNamespace(),
            loudness=types.SimpleNamespace()))
    promonet.model.discriminator = types.SimpleNamespace(
        DiscriminatorCMB=type('DiscriminatorCMB', (), dict(members)),
        DiscriminatorR=type('DiscriminatorR', (), dict(members)))
    return promonet


@pytest.mark.parametrize('name', ['DiscriminatorCMB', 'DiscriminatorR'])
def test_patch_wraps_forward_once_and_keeps_the_original(name):
    promonet = stand_in()
    cls = getattr(promonet.model.discriminator, name)
    original = cls.forward
    promonet_amd.patch(promonet)
    assert cls.forward is not original and cls.forward.original is original
    # a CPU tensor goes to the original method
    assert cls().forward(torch.zeros(1, 1, 8)) == 'forward'
    promonet_amd.patch(promonet)
    assert cls.forward.original is original


@pytest.mark.parametrize('name', ['DiscriminatorCMB', 'DiscriminatorR'])
def test_patch_leaves_a_class_without_forward_alone(name):
    promonet = stand_in(with_forward=False)
    cls = getattr(promonet.model.discriminator, name)
    promonet_amd.patch(promonet)
    assert not hasattr(cls, 'forward')
    assert hasattr(cls.spectrogram, 'original')


def test_only_the_reference_s_layer_layout_takes_the_device_path():
    def conv(*args, **kwargs):
        return torch.nn.utils.weight_norm(torch.nn.Conv2d(*args, **kwargs))

    good = types.SimpleNamespace(
        convs=[conv(1, 32, (3, 9), padding=(1, 4)),
               conv(32, 32, (3, 9), stride=(1, 2), padding=(1, 4)),
               conv(32, 32, (3, 3), padding=(1, 1))],
        conv_post=conv(32, 1, (3, 3), padding=(1, 1)))
    layers, post = discriminator._r_layers(good)
    assert [stride for _, stride in layers] == [1, 2, 1]
    assert post is good.conv_post
    for other in (
            conv(32, 32, (3, 9), stride=(2, 1), padding=(1, 4)),   # on H
            conv(32, 32, (3, 9), stride=(1, 2), padding=(4, 1)),
            conv(32, 32, (3, 9), stride=(1, 2), padding=(1, 4), dilation=2),
            conv(32, 32, (9, 3), stride=(1, 2), padding=(4, 1)),
            torch.nn.Conv2d(32, 32, (3, 9), stride=(1, 2), padding=(1, 4)),
            conv(32, 32, (3, 9), stride=(1, 2), padding=(1, 4), bias=False)):
        bad = types.SimpleNamespace(
            convs=[good.convs[0], other, good.convs[2]],
            conv_post=good.conv_post)
        assert discriminator._r_layers(bad) is None
    band = [torch.nn.Sequential(c, torch.nn.LeakyReLU(0.1))
            for c in good.convs]
    cmb = types.SimpleNamespace(band_convs=[band, band],
                                conv_post=good.conv_post)
    stacks, post = discriminator._cmb_layers(cmb)
    assert len(stacks) == 2 and stacks[0][1][1:] == (2, 0.1)
    bare = types.SimpleNamespace(band_convs=[good.convs],
                                 conv_post=good.conv_post)
    assert discriminator._cmb_layers(bare) is None
    relu = types.SimpleNamespace(
        band_convs=[[torch.nn.Sequential(c, torch.nn.ReLU())
                     for c in good.convs]], conv_post=good.conv_post)
    assert discriminator._cmb_layers(relu) is None

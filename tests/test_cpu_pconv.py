"""The conv stack of the multi-period discriminator without a GPU: the float64
oracle (tests/pconv_oracle.py) against torch's pad, view, conv2d and
leaky_relu and against the reference's own run (tests/golden/pconv.pt), the
state_dicts, the conditions the GPU tests rely on, the planted defects their
comparison must reject, the size checks and `patch()`.
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
import pconv_oracle as oracle
from conv_checks import close

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.ALL_CASES)


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'pconv.pt')


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_layer_oracle_equals_torch_in_float64(name):
    want = oracle.truth(name)
    _, y, gradients = oracle.reference_fp32(
        name, want['x'], want['weight'], want['bias'], torch.float64,
        want['upstream'])
    assert want['forward'].shape == y.shape
    assert close(want['forward'], y)
    for quantity, theirs in zip(oracle.QUANTITIES[1:], gradients):
        assert want[quantity].shape == theirs.shape
        assert close(want[quantity], theirs), quantity


def test_the_forms_are_the_module_s():
    assert oracle.FORMS == discriminator.PERIOD_FORMS
    assert {case[:4] for case in oracle.CASES.values()} == set(oracle.FORMS)
    assert oracle.SLOPE == promonet_amd.LRELU_SLOPE


def test_the_case_table_covers_what_the_issue_lists():
    for form in oracle.FORMS:
        heights = {case[4] % 3 for case in oracle.CASES.values()
                   if case[:4] == form}
        assert heights == {0, 1, 2}, form
        periods = {case[5] for case in oracle.CASES.values()
                   if case[:4] == form}
        assert periods >= {2, 3, 11}, form
    assert any(case[4] == 1 for case in oracle.CASES.values())
    assert any(case[3] == 3 and 1 < case[4] <= 3
               for case in oracle.CASES.values())
    folds = list(oracle.FOLD_CASES.values())
    assert any(samples % period == 0 for samples, period, _ in folds)
    assert any(samples == period + 1 for samples, period, _ in folds)
    assert any(oracle.reflected(samples, period) == period - 1 and
               samples > 4 * period for samples, period, _ in folds)


@pytest.mark.parametrize(
    'name', ['second-2', 'third-2', 'fourth-1', 'fifth-large'])
def test_the_large_cases_reach_past_one_tile_one_chunk_and_one_partial(name):
    """For each general kernel: a pixel count that is no multiple of the
    tile, a tile across the batch row, more than one K chunk (but at 32
    channels) with the last one, more than one gW partial"""
    channels, out_channels, kernel, stride, height, period, _ = \
        oracle.CASES[name]
    tile, chunk = oracle.CONSTANTS['PC_NT'], oracle.CONSTANTS['PC_KC']
    out_height = (height - 1) // stride + 1
    # the rows a batch row gives to the tiles of the forward, and to those of
    # gx: every input row at stride 1, a residue class at stride 3
    classes = [height] if stride == 1 else [
        len(range(r, height, 3)) for r in range(3)]
    for rows in [out_height] + classes:
        # the first tile holds all of the first batch row and some of the
        # second; the last tile is partly empty
        assert rows * period < tile and (oracle.BATCH * rows * period) % tile
    # a second tile in the forward, and in gx
    assert oracle.BATCH * out_height * period > tile
    assert any(oracle.BATCH * rows * period > tile for rows in classes)
    if name != 'second-2':
        assert channels // chunk > 1 and out_channels // chunk > 1
    chunks = math.ceil(oracle.BATCH * out_height * period /
                       oracle.CONSTANTS['PC_GW_PIX'])
    assert chunks > oracle.CONSTANTS['PC_GW_MIN_CHUNKS']
    # and the partials of the workspace say so
    library = _lib.lib()
    partial = 4 * (out_channels * channels * kernel + out_channels)
    need = library.pm_pconv_workspace_bytes(
        oracle.BATCH, channels, out_channels, height, period, kernel, stride)
    assert 2 * partial <= need < 2 * partial + 256
    one = library.pm_pconv_workspace_bytes(
        1, channels, out_channels, 1, 1, kernel, stride)
    assert partial <= one < partial + 256


def test_the_edge_cases_reach_past_one_partial():
    library = _lib.lib()
    samples, period, _ = oracle.FOLD_CASES['audio-even']
    pixels = oracle.BATCH * oracle.out_height_of('audio-even') * period
    assert pixels > oracle.CONSTANTS['PC_FOLD_CHUNK']
    assert library.pm_pconv_fold_workspace_bytes(
        oracle.BATCH, samples, period) == 2 * 4 * 192
    _, _, _, _, height, period, _ = oracle.CASES['first-2']
    assert library.pm_pconv_workspace_bytes(
        oracle.BATCH, 1, 32, height, period, 5, 3) == 2 * 4 * 192
    _, _, _, _, height, period, _ = oracle.CASES['post-2']
    parts = math.ceil(oracle.BATCH * height * period /
                      oracle.CONSTANTS['PC_POST_CHUNK'])
    assert parts > 1
    assert library.pm_pconv_workspace_bytes(
        oracle.BATCH, 1024, 1, height, period, 3, 1) == \
        math.ceil(parts * 3073 * 4 / 256) * 256


def test_the_parameters_are_exact_in_fp32():
    for key, value in oracle.parameters(2).items():
        assert value.dtype == torch.float32
        scaled = value.double() * 2 ** 14
        assert torch.equal(scaled, scaled.round())
        if key.endswith('weight_g'):
            assert value.min() >= .5
    assert not torch.equal(oracle.parameters(2)['convs.1.weight_v'],
                           oracle.parameters(5)['convs.1.weight_v'])


def stack_of(golden, period, defect=None):
    assert torch.equal(golden['audio'], oracle.stack_audio())
    return oracle.stack(
        period, golden['audio'], oracle.parameters(period), defect)


@pytest.mark.parametrize('period', oracle.PERIODS)
def test_the_stack_oracle_equals_the_reference(golden, period):
    kept = golden['stacks'][period]
    logits, maps, saved = stack_of(golden, period)
    assert kept['logits'].dtype == torch.float64
    assert [list(m.shape) for m in maps] == kept['map_shapes']
    assert len(maps) == 6
    grad_audio, gradients, _ = oracle.stack_backward(
        saved, oracle.parameters(period),
        oracle.golden_coefficients(golden, period))
    for label, _, value in oracle.stack_figures(
            golden, period, logits, maps[:-1], grad_audio, gradients):
        assert value <= 1e-12, (label, value)


def test_the_golden_audio_folds_as_the_issue_says(golden):
    samples = golden['audio'].shape[-1]
    assert [oracle.reflected(samples, p) for p in oracle.PERIODS] == [0, 4, 9]
    heights = [golden['stacks'][p]['map_shapes'] for p in oracle.PERIODS]
    assert [-(-samples // p) for p in oracle.PERIODS] == [243, 98, 45]
    assert [shapes[3][2] for shapes in heights] == [3, 2, 1]
    assert [shapes[4][2] for shapes in heights] == [3, 2, 1]


@pytest.mark.parametrize('period', oracle.PERIODS)
def test_the_mended_functional_carries_nothing_to_a_fragile_element(
        golden, period):
    _, maps, saved = stack_of(golden, period)
    mended = golden['stacks'][period]['mended']
    plain = oracle.coefficients(period, [m.shape for m in maps])
    _, _, again = oracle.stack_backward(
        saved, oracle.parameters(period), plain, mend=True)
    for mine, theirs, before in zip(
            again, oracle.golden_coefficients(golden, period), plain):
        # the same elements; the values to an ulp of fp32 (they are float64
        # sums rounded once, whose last bit may depend on the machine)
        assert torch.equal(mine != before, theirs != before)
        assert torch.allclose(mine, theirs, rtol=2. ** -22, atol=0.)
    assert 0 < len(mended[0]) < 200


@pytest.mark.parametrize('period', oracle.PERIODS)
def test_the_fragile_share_of_a_stack_is_small(golden, period):
    share = oracle.fragile_share(stack_of(golden, period)[2])
    print(f'period {period}: fragile share {share:.1e}')
    assert share <= 1e-3
    assert share == golden['stacks'][period]['fragile_share']


###############################################################################
# The state_dicts
###############################################################################


def test_discriminator_p_has_the_reference_s_keys_and_shapes(golden):
    module = discriminator.DiscriminatorP(5)
    state = module.state_dict()
    assert list(state) == golden['keys']
    assert [list(v.shape) for v in state.values()] == golden['shapes']
    assert list(oracle.shapes()) == golden['keys']
    parameters = oracle.parameters(5)
    module.load_state_dict(parameters, strict=True)
    key = golden['keys'][-4]
    assert torch.equal(module.state_dict()[key], parameters[key])


def test_the_aggregate_has_the_default_configuration_s_keys_and_shapes(
        golden):
    module = discriminator.Discriminator()
    state = module.state_dict()
    assert list(state) == golden['discriminator_keys']
    assert [list(v.shape) for v in state.values()] == \
        golden['discriminator_shapes']
    module.load_state_dict(
        {key: torch.full(shape, .25) for key, shape in zip(
            golden['discriminator_keys'], golden['discriminator_shapes'])},
        strict=True)
    assert [type(m).__name__ for m in module.discriminators] == \
        ['DiscriminatorP'] * 5 + ['DiscriminatorCMB']
    assert [m.period for m in module.discriminators[:5]] == [2, 3, 5, 7, 11]
    other = discriminator.Discriminator(
        (3,), False, [(512, 50, 240), (1024, 120, 600)])
    assert [type(m).__name__ for m in other.discriminators] == \
        ['DiscriminatorP', 'DiscriminatorR', 'DiscriminatorR']


###############################################################################
# What the GPU tests rely on
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_fragile_share_is_small(name):
    conv_checks.the_fragile_share_is_small(oracle, name)


@pytest.mark.parametrize('name', NAMES)
def test_the_gates_come_from_the_reference_arithmetic_in_fp32(name):
    assert set(oracle.FP32_RECORDED) == set(oracle.ALL_CASES)
    conv_checks.the_gates_come_from_the_reference_arithmetic_in_fp32(
        oracle, name)


@pytest.mark.parametrize('shape', oracle.WEIGHT_NORM_SHAPES)
def test_the_weight_norm_gates_come_from_torch_in_fp32(shape):
    conv_checks.the_weight_norm_gates_come_from_torch_in_fp32(oracle, shape)
    assert sorted(math.prod(s[1:]) for s in oracle.WEIGHT_NORM_SHAPES) == \
        [5, 160, 640, 2560, 3072, 5120]


###############################################################################
# Planted defects: the comparison of the GPU tests (the shapes and the four
# figures against the gates) rejects each of them in every case it can touch
###############################################################################

MAPS = list(oracle.CASES)
FOLDS = list(oracle.FOLD_CASES)
STRIDED = [n for n in MAPS if oracle.CASES[n][3] == 3]
SLOPED = [n for n in NAMES if oracle.form_of(n)[4] != 1.]
PADDED = [n for n in FOLDS if oracle.reflected(*oracle.FOLD_CASES[n][:2])]
APPLIES = {
    'stride_on_width': STRIDED,
    # (a height of 1 reads the centre tap alone, whatever the padding and
    # the order of the taps)
    'padding_one_at_k5': [n for n in MAPS if oracle.CASES[n][2] == 5 and
                          oracle.CASES[n][4] > 1],
    'height_rounded_up': [n for n in STRIDED if not oracle.CASES[n][4] % 3],
    'taps_flipped': [n for n in MAPS if oracle.CASES[n][4] > 1],
    # (one row above or below to read: a height of 1 has its taps in the
    # padding of both neighbours)
    'tap_across_batch_row': [n for n in MAPS if oracle.CASES[n][4] > 1],
    'tap_from_neighbour_column': [n for n in MAPS if oracle.CASES[n][4] > 1],
    # (a second tap: an input row 3 j + 1 or 3 j + 2 with an output row j)
    'gx_second_tap_dropped': [n for n in STRIDED if oracle.CASES[n][4] > 1],
    # (where the last window reaches it: not at stride 3 and H = 3 m, whose
    # last window ends on the last row)
    'gw_bottom_rows_dropped': [
        n for n in MAPS if oracle.CASES[n][4] > 1 and
        (oracle.CASES[n][3] == 1 or oracle.CASES[n][4] % 3)],
    'slope_on_positive': SLOPED,
    'slope_left_out_of_gz': SLOPED,
    'mask_from_input': SLOPED,
    'fold_axes_swapped': [n for n in FOLDS if n != 'audio-short'],
    'zero_pad': PADDED,
    'reflect_repeats_edge': PADDED,
    'reflect_adjoint_left_out': PADDED,
}


def accepted(name, defect):
    """Would the GPU tests pass an implementation with this defect?"""
    return conv_checks.accepted(
        oracle, name, lambda *inputs: oracle.case_layer(name, *inputs, defect),
        lambda *inputs: oracle.case_backward(name, *inputs, defect))


def test_the_defects_are_all_listed():
    assert set(APPLIES) == set(oracle.DEFECTS) | set(oracle.FOLD_DEFECTS)
    assert all(APPLIES.values())
    assert len(APPLIES) + len(oracle.STACK_DEFECTS) == 17


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_itself_is_accepted(name):
    assert accepted(name, None)


@pytest.mark.parametrize(
    'defect,name',
    [(defect, name) for defect in APPLIES for name in APPLIES[defect]])
def test_a_planted_defect_is_rejected(defect, name):
    assert not accepted(name, defect)


def stack_accepted(golden, period, defect):
    logits, maps, saved = stack_of(golden, period, defect)
    grad_audio, gradients, _ = oracle.stack_backward(
        saved, oracle.parameters(period),
        oracle.golden_coefficients(golden, period))
    return all(value < oracle.gate(quantity) for _, quantity, value in
               oracle.stack_figures(golden, period, logits, maps[:-1],
                                    grad_audio, gradients))


@pytest.mark.parametrize('period', oracle.PERIODS)
def test_the_stack_oracle_itself_is_accepted(golden, period):
    assert stack_accepted(golden, period, None)


@pytest.mark.parametrize('period', oracle.PERIODS)
@pytest.mark.parametrize('defect', oracle.STACK_DEFECTS)
def test_a_planted_stack_defect_is_rejected(golden, defect, period):
    assert not stack_accepted(golden, period, defect)


###############################################################################
# Sizes: ValueError from Python, PM_EINVAL from the ABI, no device needed
###############################################################################


def arguments(channels=32, out_channels=128, kernel=5, height=7, period=3):
    return (torch.zeros(2, channels, height, period),
            torch.zeros(out_channels, channels, kernel, 1),
            torch.zeros(out_channels))


BAD = [
    (lambda x, w, b: (x[0], w, b), {'stride': 3}),                # not 4-D
    (lambda x, w, b: (x[:, :16], w[:, :16], b), {'stride': 3}),   # C = 16
    (lambda x, w, b: (x, w[:64], b[:64]), {'stride': 3}),         # O = 64
    (lambda x, w, b: (x[:, :1], w, b), {'stride': 3}),            # C of x
    (lambda x, w, b: (x, w[:, :, :3], b), {'stride': 3}),         # k = 3
    (lambda x, w, b: (x, w.expand(-1, -1, -1, 2), b), {'stride': 3}),
    (lambda x, w, b: (x, w[..., 0], b), {'stride': 3}),           # 3-D weight
    (lambda x, w, b: (x, w, b[:1]), {'stride': 3}),               # bias
    (lambda x, w, b: (x[:, :, :0], w, b), {'stride': 3}),         # empty
    (lambda x, w, b: (x.long(), w, b), {'stride': 3}),            # not float
    (lambda x, w, b: (x, w, b), {'stride': 1}),                   # (32,128,5,1)
    (lambda x, w, b: (x, w, b), {'stride': 2}),
    (lambda x, w, b: (x, w, b), {'stride': (1, 3)}),              # on P
    (lambda x, w, b: (x[..., :1].expand(-1, -1, -1, 65), w, b),
     {'stride': 3}),                                              # P = 65
    (lambda x, w, b: (x, w, b), {'stride': 3, 'slope': 0.}),
    (lambda x, w, b: (x, w, b), {'stride': 3, 'slope': 1.5}),
    (lambda x, w, b: (x, w, b), {'stride': 3, 'slope': -.1}),
    (lambda x, w, b: (x, w, b), {'stride': 3, 'slope': float('nan')}),
    (lambda x, w, b: (x, w, b), {'stride': 3, 'slope': float('inf')}),
    (lambda x, w, b: (x, w, b), {'stride': 3, 'slope': 'leaky'}),
]


@pytest.mark.parametrize('change,keywords', BAD)
def test_bad_arguments_raise_before_any_device_work(change, keywords):
    with pytest.raises(ValueError):
        discriminator.period_conv(*change(*arguments()), **keywords)


def fold_arguments(samples=100):
    return (torch.zeros(2, 1, samples), torch.zeros(32, 1, 5, 1),
            torch.zeros(32))


FOLD_BAD = [
    (lambda a, w, b: (a[0, 0], w, b), {'period': 3}),             # 1-D
    (lambda a, w, b: (a.expand(-1, 2, -1), w, b), {'period': 3}),
    (lambda a, w, b: (a[..., :0], w, b), {'period': 3}),          # empty
    (lambda a, w, b: (a.long(), w, b), {'period': 3}),
    (lambda a, w, b: (a, w[:16], b[:16]), {'period': 3}),         # O = 16
    (lambda a, w, b: (a, w[:, :, :3], b), {'period': 3}),         # k = 3
    (lambda a, w, b: (a, w, b[:1]), {'period': 3}),
    (lambda a, w, b: (a, w, b), {'period': 0}),
    (lambda a, w, b: (a, w, b), {'period': 65}),
    (lambda a, w, b: (a, w, b), {'period': 2.}),
    (lambda a, w, b: (a, w, b), {'period': True}),
    # samples <= n: 4 samples at period 5 reflect 1 ... and 1 sample at
    # period 3 reflects 2, as torch refuses it
    (lambda a, w, b: (a[..., :1], w, b), {'period': 3}),
    (lambda a, w, b: (a[..., :3], w, b), {'period': 7}),
    (lambda a, w, b: (a, w, b), {'period': 3, 'slope': 0.}),
    (lambda a, w, b: (a, w, b), {'period': 3, 'slope': float('nan')}),
    (lambda a, w, b: (a, w, b), {'period': 3, 'slope': 2}),
]


def test_more_than_2_31_pixels_are_refused_before_any_device_work():
    """(views of one element: nothing that large is allocated)"""
    x, weight, bias = arguments()
    with pytest.raises(ValueError, match='pixels'):
        discriminator.period_conv(
            x[:1, :, :1, :1].expand(1 << 16, -1, 1 << 15, 1), weight, bias,
            stride=3)
    audio, weight, bias = fold_arguments()
    with pytest.raises(ValueError, match='pixels'):
        discriminator.period_fold_conv(
            audio[:1, :, :1].expand(1 << 11, -1, 1 << 20), weight, bias,
            period=2)


@pytest.mark.parametrize('change,keywords', FOLD_BAD)
def test_bad_fold_arguments_raise_before_any_device_work(change, keywords):
    with pytest.raises(ValueError):
        discriminator.period_fold_conv(
            *change(*fold_arguments()), **keywords)


def test_torch_refuses_the_same_short_audio():
    with pytest.raises(RuntimeError):
        oracle.reference_fold(torch.zeros(2, 1, 3), 7)
    oracle.reference_fold(torch.zeros(2, 1, 4), 7)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.period_fold_conv(
            *fold_arguments(4), period=7, slope=.1)


@pytest.mark.parametrize('form', oracle.FORMS)
def test_good_sizes_on_a_cpu_tensor_say_that_there_is_no_fallback(form):
    channels, out_channels, kernel, stride = form
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.period_conv(
            *arguments(channels, out_channels, kernel), stride=stride,
            slope=.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.period_conv(
            *arguments(channels, out_channels, kernel), stride=(stride, 1))


def test_the_fold_and_the_modules_on_a_cpu_tensor_say_the_same():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.period_fold_conv(*fold_arguments(), period=3, slope=.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.period_fold_conv(
            fold_arguments()[0][:, 0], *fold_arguments()[1:], 64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.DiscriminatorP(3)(torch.zeros(2, 1, 100))
    with pytest.raises(ValueError):
        discriminator.DiscriminatorP(0)
    with pytest.raises(ValueError):
        discriminator.DiscriminatorP(3)(torch.zeros(2, 1, 1))


GOOD_SIZES = (2, 32, 128, 7, 3, 5, 3)
ABI_BAD = [
    # batch, channels, out_channels, height, period, kernel, stride
    ((2, 16, 128, 7, 3, 5, 3), .1),
    ((2, 32, 64, 7, 3, 5, 3), .1),
    ((2, 32, 128, 7, 3, 3, 3), .1),
    ((2, 32, 128, 7, 3, 5, 1), .1),
    ((2, 32, 128, 7, 3, 5, 0), .1),
    ((2, 1, 32, 7, 3, 5, 1), .1),
    ((2, 1, 1, 7, 3, 3, 1), .1),
    ((2, 128, 512, 7, 3, 5, 1), .1),
    ((2, 512, 1024, 7, 3, 5, 1), .1),
    ((2, 1024, 1024, 7, 3, 5, 3), .1),
    ((2, 1024, 1024, 7, 3, 3, 1), .1),
    ((2, 1024, 1, 7, 3, 5, 1), .1),
    ((2, 1024, 1, 7, 3, 3, 3), .1),
    ((0, 32, 128, 7, 3, 5, 3), .1),
    ((2, 32, 128, 0, 3, 5, 3), .1),
    ((2, 32, 128, 7, 0, 5, 3), .1),
    ((2, 32, 128, 7, 65, 5, 3), .1),
    ((2, 32, 128, 7, -1, 5, 3), .1),
    ((1 << 20, 32, 128, 1 << 20, 64, 5, 3), .1),        # 2^46 pixels
    ((1 << 10, 32, 128, 1 << 15, 64, 5, 3), .1),        # 2^31 input pixels
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
        assert library.pm_pconv_workspace_bytes(*sizes) == 0
    # (the pointers are never read: the sizes are refused first)
    code = library.pm_pconv_forward(256, 256, 256, 256, *sizes, slope, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_pconv_forward' in library.pm_last_error()
    code = library.pm_pconv_backward(
        256, 256, 256, 256, 256, 256, 256, *sizes, slope, 256, 1 << 40, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_pconv_backward' in library.pm_last_error()


GOOD_FOLD = (2, 100, 3)
FOLD_ABI_BAD = [
    # batch, samples, period
    ((0, 100, 3), .1),
    ((2, 0, 3), .1),
    ((2, 100, 0), .1),
    ((2, 100, 65), .1),
    ((2, 1, 3), .1),                    # 2 reflected samples of 1
    ((2, 3, 7), .1),                    # 4 of 3
    ((2, 6, 13), .1),                   # 7 of 6
    ((1 << 10, 1 << 21, 64), .1),       # 2^31 pixels
    (GOOD_FOLD, 0.),
    (GOOD_FOLD, 1.5),
    (GOOD_FOLD, float('nan')),
    (GOOD_FOLD, float('-inf')),
]


@pytest.mark.parametrize('sizes,slope', FOLD_ABI_BAD)
def test_the_abi_refuses_bad_fold_sizes_on_the_host(sizes, slope):
    library = _lib.lib()
    if sizes != GOOD_FOLD:
        assert library.pm_pconv_fold_workspace_bytes(*sizes) == 0
    code = library.pm_pconv_fold_forward(
        256, 256, 256, 256, *sizes, slope, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_pconv_fold_forward' in library.pm_last_error()
    code = library.pm_pconv_fold_backward(
        256, 256, 256, 256, 256, 256, 256, *sizes, slope, 256, 1 << 40, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_pconv_fold_backward' in library.pm_last_error()


def refuses_pointers(forward, backward, name, sizes, need):
    library = _lib.lib()
    for null in range(4):
        pointers = [256] * 4
        pointers[null] = None
        code = forward(*pointers, *sizes, .1, None)
        assert code == _lib.PM_EINVAL
        assert name + b'_forward' in library.pm_last_error()
    for null in (0, 1, 2, 3, 5, 6):
        pointers = [256] * 7
        pointers[null] = None
        code = backward(*pointers, *sizes, .1, 256, need, None)
        assert code == _lib.PM_EINVAL
        assert name + b'_backward' in library.pm_last_error()
    code = backward(*[256] * 7, *sizes, .1, None, need, None)
    assert code == _lib.PM_EINVAL
    code = backward(*[256] * 7, *sizes, .1, 256, need - 1, None)
    assert code == _lib.PM_ENOMEM
    assert name + b'_backward' in library.pm_last_error()


@pytest.mark.parametrize('form', oracle.FORMS)
def test_the_abi_refuses_null_pointers_and_a_small_workspace(form):
    library = _lib.lib()
    channels, out_channels, kernel, stride = form
    sizes = (2, channels, out_channels, 7, 3, kernel, stride)
    need = library.pm_pconv_workspace_bytes(*sizes)
    assert need >= 4 * (channels * out_channels * kernel + out_channels) \
        and need % 256 == 0
    refuses_pointers(library.pm_pconv_forward, library.pm_pconv_backward,
                     b'pm_pconv', sizes, need)


def test_the_fold_abi_refuses_null_pointers_and_a_small_workspace():
    library = _lib.lib()
    need = library.pm_pconv_fold_workspace_bytes(*GOOD_FOLD)
    assert need == 4 * 192
    refuses_pointers(
        library.pm_pconv_fold_forward, library.pm_pconv_fold_backward,
        b'pm_pconv_fold', GOOD_FOLD, need)


def test_the_workspace_stays_modest_at_the_training_shape():
    """batch 64 x 16 384 samples: at most PC_GW_WORKGROUPS workgroups of gW,
    tiles x partials, so a layer's partials stay under 64 MB"""
    library = _lib.lib()
    for period in discriminator.PERIODS:
        height = -(-16384 // period)
        assert 0 < library.pm_pconv_fold_workspace_bytes(
            64, 16384, period) <= \
            oracle.CONSTANTS['PC_EDGE_MAX_PARTS'] * 4 * 192
        for channels, out_channels, kernel, stride in oracle.FORMS:
            need = library.pm_pconv_workspace_bytes(
                64, channels, out_channels, height, period, kernel, stride)
            assert 0 < need <= 64 << 20
            height = (height - 1) // stride + 1


###############################################################################
# patch()
###############################################################################


def stand_in(with_forward=True):
    members = {}
    if with_forward:
        members['forward'] = lambda self, x: 'forward'
    promonet = types.SimpleNamespace(
        model=types.SimpleNamespace(HiFiGAN=None, FARGAN=None, Generator=None),
        synthesize=types.SimpleNamespace(),
        preprocess=types.SimpleNamespace(
            spectrogram=types.SimpleNamespace(),
            loudness=types.SimpleNamespace()))
    promonet.model.discriminator = types.SimpleNamespace(
        DiscriminatorP=type('DiscriminatorP', (), dict(members)))
    return promonet


def test_patch_wraps_forward_once_and_keeps_the_original():
    promonet = stand_in()
    cls = promonet.model.discriminator.DiscriminatorP
    original = cls.forward
    promonet_amd.patch(promonet)
    assert cls.forward is not original and cls.forward.original is original
    # a CPU tensor goes to the original method
    assert cls().forward(torch.zeros(1, 1, 8)) == 'forward'
    promonet_amd.patch(promonet)
    assert cls.forward.original is original


def test_patch_leaves_a_class_without_forward_alone():
    promonet = stand_in(with_forward=False)
    promonet_amd.patch(promonet)
    assert not hasattr(promonet.model.discriminator.DiscriminatorP, 'forward')


def conv(*args, **kwargs):
    return torch.nn.utils.weight_norm(torch.nn.Conv2d(*args, **kwargs))


def reference_layout(period=3, **changes):
    """The layers of the reference's DiscriminatorP; `changes` replaces
    convs.{index} or conv_post"""
    convs = [conv(c, o, (k, 1), (s, 1), padding=((k - 1) // 2, 0))
             for c, o, k, s in oracle.FORMS[:5]]
    post = conv(1024, 1, (3, 1), 1, padding=(1, 0))
    for key, value in changes.items():
        if key == 'post':
            post = value
        else:
            convs[int(key[1:])] = value
    return types.SimpleNamespace(
        period=period, convs=torch.nn.ModuleList(convs), conv_post=post)


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_only_the_reference_s_layer_layout_takes_the_device_path():
    good = reference_layout()
    convs, post, period = discriminator._p_layers(good)
    assert len(convs) == 5 and post is good.conv_post and period == 3
    for changes in (
            # the stride on W
            {'c1': conv(32, 128, (5, 1), (1, 3), padding=(2, 0))},
            {'c1': conv(32, 128, (5, 1), (3, 3), padding=(2, 0))},
            # the kernel and the padding on W
            {'c1': conv(32, 128, (1, 5), (3, 1), padding=(0, 2))},
            {'c1': conv(32, 128, (5, 1), (3, 1), padding=(2, 1))},
            {'c1': conv(32, 128, (5, 1), (3, 1), padding=(1, 0))},
            {'c1': conv(32, 128, (5, 1), (3, 1), padding=(2, 0), dilation=2)},
            {'c1': conv(32, 128, (5, 1), (3, 1), padding=(2, 0), bias=False)},
            {'c1': torch.nn.Conv2d(32, 128, (5, 1), (3, 1), padding=(2, 0))},
            {'c4': conv(1024, 1024, (5, 1), (3, 1), padding=(2, 0))},
            {'c0': conv(1, 32, (5, 1), (3, 1), padding=(2, 0), groups=1,
                        padding_mode='reflect')},
            {'post': conv(1024, 1, (3, 1), 1, padding=(0, 0))},
            {'post': conv(1024, 1, (5, 1), 1, padding=(2, 0))}):
        assert discriminator._p_layers(reference_layout(**changes)) is None
    assert discriminator._p_layers(reference_layout(period=0)) is None
    assert discriminator._p_layers(reference_layout(period=2.)) is None
    short = reference_layout()
    short.convs = short.convs[:4]
    assert discriminator._p_layers(short) is None
    assert discriminator._p_layers(types.SimpleNamespace()) is None


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_a_stand_in_with_the_stride_on_w_goes_to_the_original():
    calls = []

    class DiscriminatorP(torch.nn.Module):

        def __init__(self):
            super().__init__()
            self.period = 3
            self.convs = torch.nn.ModuleList(
                [conv(1, 2, (5, 1), (1, 3), padding=(2, 0))])
            self.conv_post = conv(2, 1, (3, 1), 1, padding=(1, 0))

        def forward(self, x):
            calls.append(tuple(x.shape))
            return 'theirs'

    module = types.SimpleNamespace(DiscriminatorP=DiscriminatorP)
    discriminator.patch_module(module)
    discriminator.patch_module(module)
    assert DiscriminatorP.forward.original.__qualname__.endswith(
        'DiscriminatorP.forward')
    assert DiscriminatorP()(torch.zeros(2, 1, 30)) == 'theirs'
    assert calls == [(2, 1, 30)]

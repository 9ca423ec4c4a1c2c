"""The convs of the generator's MRF Blocks without a GPU: the float64 oracle
(tests/gconv_oracle.py) against torch's leaky_relu and conv1d and against the
reference's own run (tests/golden/gconv.pt), the state_dicts, the conditions
the GPU tests rely on, the planted defects their comparison must reject, the
size checks and `patch()`.
"""
import types
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.model import hifigan_train

import gconv_oracle as oracle
from conv_checks import close

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'gconv.pt')


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_layer_oracle_equals_torch_in_float64(name):
    for slope in oracle.SLOPES:
        want = oracle.truth(name, slope)
        y, gradients = oracle.reference(
            want['x'], want['weight'], want['bias'], oracle.CASES[name][2],
            slope, want['residual'], want['upstream'], torch.float64)
        assert want['forward_residual'].shape == y.shape
        assert close(want['forward_residual'], y)
        for quantity, theirs in zip(oracle.QUANTITIES[1:], gradients):
            assert want[quantity].shape == theirs.shape
            assert close(want[quantity], theirs), quantity


def test_the_forms_are_the_module_s():
    assert oracle.CHANNELS == hifigan_train.CHANNELS
    assert oracle.KERNELS == hifigan_train.KERNELS
    assert oracle.DILATIONS == hifigan_train.DILATIONS
    assert oracle.SLOPE == promonet_amd.LRELU_SLOPE
    assert oracle.BLOCKS == tuple(zip(
        promonet_amd.HIFIGAN_RESBLOCK_KERNEL_SIZES,
        map(tuple, promonet_amd.HIFIGAN_RESBLOCK_DILATION_SIZES)))
    assert oracle.CONSTANTS['GC_MAX_DILATION'] == max(oracle.DILATIONS)


def test_the_case_table_covers_what_the_issue_lists():
    cases = set(oracle.CASES.values())
    for channels in oracle.CHANNELS:
        for kernel in oracle.KERNELS:
            for dilation in oracle.DILATIONS:
                assert (channels, kernel, dilation, 2, 37) in cases
    for case in ((32, 11, 5, 2, 1), (32, 11, 5, 2, 5), (256, 3, 1, 2, 1),
                 (256, 3, 1, 2, 5), (64, 11, 5, 2, 25), (64, 11, 5, 2, 26)):
        assert case in cases
    assert (11 - 1) // 2 * 5 == 25
    assert set(oracle.SLOPES) == {.1, 1.}
    assert set(oracle.EXACT_SLOPES) == {.5, 1.}
    for name in NAMES:
        x = oracle.truth(name, oracle.SLOPE)['x']
        assert (x == 0.).any() and (x > 0.).any() and (x < 0.).any()


@pytest.mark.parametrize('name', ['large-32', 'large-128'])
def test_the_large_cases_reach_past_one_tile_one_chunk_and_one_partial(name):
    """A frame count 16 n +- 1 past one pixel tile of the forward and of gx
    (so the tiles cross the batch rows, and the last is partly empty), one K
    chunk of gW and one gW partial; more than one K chunk of the forward at
    128 channels"""
    channels, kernel, _, batch, frames = oracle.CASES[name]
    assert batch == 3 and 340 <= frames <= 360 and frames % 16 in (1, 15)
    tile, pixels = oracle.CONSTANTS['GC_NT'], oracle.CONSTANTS['GC_GW_PIX']
    assert frames > tile and frames % tile and (batch * frames) % tile
    assert frames > pixels and (batch * frames) % pixels
    parts, each = oracle.split(batch, channels, frames)
    assert parts > 1 and frames > each * pixels
    assert each >= oracle.CONSTANTS['GC_GW_MIN_CHUNKS']
    if name == 'large-128':
        assert channels // oracle.CONSTANTS['GC_KC'] > 1
    # and the partials of the workspace say so
    library = _lib.lib()
    partial = 4 * (channels * channels * kernel + channels)
    need = library.pm_gconv_workspace_bytes(
        batch, channels, frames, kernel, oracle.CASES[name][2])
    assert parts * partial <= need < parts * partial + 256
    one = library.pm_gconv_workspace_bytes(1, channels, 1, kernel, 1)
    assert partial <= one < partial + 256


@pytest.mark.parametrize('name', NAMES)
def test_the_reference_arithmetic_in_fp32_stays_inside_the_gates(name):
    """The gates are 4 x the recorded figures; the figures of this machine
    are within them (and, on the build host, equal to the record)"""
    figures = oracle.fp32_figures(name)
    print(f"    '{name}': (" + ', '.join(f'{v:.3e}' for v in figures) + '),')
    for quantity, value in zip(oracle.QUANTITIES, figures):
        assert value < oracle.gate(quantity), (quantity, value)


###############################################################################
# The planted defects
###############################################################################


def defective(name, slope, defect):
    """(y with the residual, gx, gW, gb) of the oracle with a defect planted"""
    want = oracle.truth(name, slope)
    dilation = oracle.CASES[name][2]
    y = oracle.layer(want['x'], want['weight'], want['bias'], dilation, slope,
                     want['residual'], defect)
    return (y,) + oracle.layer_backward(
        want['x'], want['weight'], want['upstream'], dilation, slope, defect,
        y=want['forward'])


def rejected(name, slope, results):
    figures = oracle.figures(name, slope, *results, residual=True)
    return [quantity for quantity, value in zip(oracle.QUANTITIES, figures)
            if not value < oracle.gate(quantity)]


@pytest.mark.parametrize('name', ['form-32-3-3', 'form-64-11-5', 'large-32'])
def test_the_comparison_accepts_the_oracle(name):
    assert not rejected(name, oracle.SLOPE, defective(name, oracle.SLOPE, None))


@pytest.mark.parametrize('defect,quantity', [
    ('gx_dilation_ignored', 'gx'), ('gx_taps_not_mirrored', 'gx'),
    ('gate_from_output', 'gx'), ('zero_gated_as_one', 'gx'),
    ('slope_left_out_of_gw', 'gW'), ('padding_reads_neighbour', 'forward'),
    ('padding_reads_neighbour', 'gW'), ('residual_twice', 'forward')])
def test_the_comparison_rejects_a_planted_layer_defect(defect, quantity):
    assert defect in oracle.LAYER_DEFECTS
    for name in ('form-32-3-3', 'form-64-11-5', 'large-32'):
        assert quantity in rejected(
            name, oracle.SLOPE, defective(name, oracle.SLOPE, defect)), name


def module_rejected(name, defect):
    forward, parameters = oracle.module_case(name)
    want = oracle.module_truth(name)
    planted = oracle.module_truth(name, defect)
    figures = oracle.module_figures(
        name, planted['forward'], planted['gx'], planted['gradients'])
    assert planted is not want or defect is None
    return [index for index, (value, limit) in enumerate(
        zip(figures, oracle.module_gates())) if not value < limit]


def test_the_comparison_rejects_a_planted_module_defect():
    assert not module_rejected('block-7', None)
    assert not module_rejected('residual', None)
    # the skip's gradient dropped: the forward is right, the gradients are not
    assert module_rejected('block-7', 'residual_gradient_dropped') == [1, 2, 3]
    assert 0 in module_rejected('block-7', 'conv2_dilated')
    assert 0 in module_rejected('residual', 'no_division')
    assert 0 in module_rejected('residual', 'kernels_permuted')
    assert set(oracle.MODULE_DEFECTS) == {
        'residual_gradient_dropped', 'conv2_dilated', 'no_division',
        'kernels_permuted'}


###############################################################################
# The modules
###############################################################################


@pytest.mark.parametrize('name', list(oracle.MODULE_SEEDS))
def test_no_leaky_input_of_a_module_case_is_fragile(name):
    """So the fp32 reference and the device cannot disagree on a mask"""
    assert oracle.fragile_bound() == pytest.approx(64 * 1.404e-06)
    assert oracle.module_truth(name)['fragile'] == 0


@pytest.mark.parametrize('name', list(oracle.MODULE_SEEDS))
def test_the_module_composition_in_fp32_stays_inside_the_gates(name):
    figures = oracle.module_figures(name, *oracle.module_reference(name))
    print(f"    '{name}': (" + ', '.join(f'{v:.3e}' for v in figures) + '),')
    for value, limit in zip(figures, oracle.module_gates()):
        assert value < limit, (value, limit)
    exact = oracle.module_figures(
        name, *oracle.module_reference(name, torch.float64))
    assert max(exact) < 1e-12


@pytest.mark.parametrize('kernel', oracle.KERNELS)
def test_the_oracle_composition_equals_the_reference_s_block(golden, kernel):
    kept = golden['blocks'][kernel]
    want = oracle.module_truth(f'block-{kernel}')
    assert torch.equal(kept['x'], want['x'])
    assert torch.equal(kept['upstream'], want['upstream'])
    assert close(want['forward'], kept['forward'])
    assert close(want['gx'], kept['gx'])
    assert [key for key, _ in kept['gradient_counts']] == kept['keys']
    pieces = kept['gradients'].split(
        [count for _, count in kept['gradient_counts']])
    for key, piece in zip(kept['keys'], pieces):
        step = golden['gradient_stride'] if key.endswith('weight_v') else 1
        assert close(want['gradients'][key].flatten()[::step], piece), key


def shapes_of(module):
    state = module.state_dict()
    return list(state), [list(value.shape) for value in state.values()]


def test_the_state_dicts_are_the_reference_s(golden):
    for kernel, dilations in oracle.BLOCKS:
        kept = golden['blocks'][kernel]
        module = hifigan_train.Block(oracle.MODULE_CHANNELS, kernel, dilations)
        assert shapes_of(module) == (kept['keys'], kept['shapes'])
        assert list(oracle.block_shapes(
            oracle.MODULE_CHANNELS, kernel).items()) == [
                (key, tuple(shape))
                for key, shape in zip(kept['keys'], kept['shapes'])]
    assert shapes_of(hifigan_train.ResidualBlock(oracle.MODULE_CHANNELS)) == (
        golden['residual_keys'], golden['residual_shapes'])
    assert list(oracle.residual_shapes(oracle.MODULE_CHANNELS)) == \
        golden['residual_keys']
    trainable = hifigan_train.HiFiGANTrainable(113, 258)
    assert shapes_of(trainable) == (
        golden['hifigan_keys'], golden['hifigan_shapes'])
    assert all(p.requires_grad for p in trainable.parameters())
    engine = promonet_amd.model.HiFiGAN(113, 258)
    assert shapes_of(engine) == shapes_of(trainable)
    engine.load_state_dict(trainable.state_dict(), strict=True)
    trainable.load_state_dict(engine.state_dict(), strict=True)
    state = oracle.trainable_state()
    assert list(state) == golden['hifigan_keys']
    trainable.load_state_dict(state, strict=True)


def test_the_vocoder_restatement_in_fp32_stays_inside_the_gates():
    """(float64 and fp32 with autograd on the CPU: a second or so)"""
    figures = oracle.trainable_figures(*oracle.trainable_run(torch.float32))
    print('TRAINABLE_RECORDED = (' +
          ', '.join(f'{v:.3e}' for v in figures) + ')')
    assert len(figures) == len(oracle.TRAINABLE_QUANTITIES)
    for value, limit in zip(figures, oracle.trainable_gates()):
        assert value < limit, (value, limit)
    # stage 1 has 16 steps, shorter than a Block's reach
    assert oracle.TRAINABLE_FRAMES * 8 < 2 * 25


def test_the_parameters_are_exact_in_fp32():
    for key, value in oracle.module_case('residual')[1].items():
        assert value.dtype == torch.float32
        scaled = value.double() * 2 ** 14
        assert torch.equal(scaled, scaled.round())


###############################################################################
# ValueErrors before any device work
###############################################################################


def arguments(channels=32, kernel=3, frames=9):
    return (torch.zeros(2, channels, frames),
            torch.zeros(channels, channels, kernel), torch.zeros(channels))


BAD = [
    (lambda x, w, b: (x[0], w, b), {}),                           # 2-D
    (lambda x, w, b: (x[..., :0], w, b), {}),                     # empty
    (lambda x, w, b: (x.long(), w, b), {}),
    (lambda x, w, b: (x, w.long(), b), {}),
    (lambda x, w, b: (x[:, :16], w, b), {}),
    (lambda x, w, b: (x, w[:16], b[:16]), {}),                    # O = 16
    (lambda x, w, b: (x[:, :16], w[:16, :16], b[:16]), {}),       # C = 16
    (lambda x, w, b: (x, w[:, :, :2], b), {}),                    # k = 2
    (lambda x, w, b: (x, w[..., None], b), {}),
    (lambda x, w, b: (x, w, b[:1]), {}),
    (lambda x, w, b: (x, w, b), {'dilation': 2}),
    (lambda x, w, b: (x, w, b), {'dilation': 0}),
    (lambda x, w, b: (x, w, b), {'dilation': True}),
    (lambda x, w, b: (x, w, b), {'dilation': (1, 3)}),
    (lambda x, w, b: (x, w, b), {'slope': 0.}),
    (lambda x, w, b: (x, w, b), {'slope': float('nan')}),
    (lambda x, w, b: (x, w, b), {'slope': 2}),
    (lambda x, w, b: (x, w, b), {'slope': True}),
    (lambda x, w, b: (x, w, b), {'residual': torch.zeros(2, 32, 8)}),
    (lambda x, w, b: (x, w, b), {'residual': torch.zeros(2, 32, 9).long()}),
]


@pytest.mark.parametrize('change,keywords', BAD)
def test_bad_arguments_raise_before_any_device_work(change, keywords):
    with pytest.raises(ValueError):
        hifigan_train.block_conv(*change(*arguments()), **keywords)


def test_more_than_2_31_pixels_are_refused_before_any_device_work():
    """(a view of one element: nothing that large is allocated)"""
    x, weight, bias = arguments()
    with pytest.raises(ValueError, match='pixels'):
        hifigan_train.block_conv(
            x[:1, :, :1].expand(1 << 16, -1, 1 << 15), weight, bias)


@pytest.mark.parametrize('channels', oracle.CHANNELS)
def test_good_sizes_on_a_cpu_tensor_say_that_there_is_no_fallback(channels):
    for kernel in oracle.KERNELS:
        for dilation in oracle.DILATIONS:
            x, weight, bias = arguments(channels, kernel)
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                hifigan_train.block_conv(
                    x, weight, bias, dilation, 1., residual=x)


def test_the_modules_refuse_other_forms_and_say_the_same():
    for args in ((48, 3), (32, 5), (32, 3, (1, 2, 4)), (32, 3, ())):
        with pytest.raises(ValueError):
            hifigan_train.Block(*args)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hifigan_train.Block(32, 3)(torch.zeros(2, 32, 9))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hifigan_train.ResidualBlock(32)(torch.zeros(2, 32, 9))
    with pytest.raises(ValueError):
        hifigan_train.ResidualBlock(32)(torch.zeros(2, 32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hifigan_train.HiFiGANTrainable(113, 258)(
            torch.zeros(2, 113, 2), torch.zeros(2, 258, 1))
    assert promonet_amd.model.HiFiGANTrainable is \
        hifigan_train.HiFiGANTrainable
    assert promonet_amd.model.block_conv is hifigan_train.block_conv


###############################################################################
# The C ABI on the host
###############################################################################

GOOD_SIZES = (2, 64, 37, 7, 3)
ABI_BAD = [
    # batch, channels, frames, kernel, dilation
    ((2, 16, 37, 7, 3), .1),
    ((2, 48, 37, 7, 3), .1),
    ((2, 512, 37, 7, 3), .1),
    ((2, 64, 37, 5, 3), .1),
    ((2, 64, 37, 1, 3), .1),
    ((2, 64, 37, 13, 3), .1),
    ((2, 64, 37, 7, 2), .1),
    ((2, 64, 37, 7, 0), .1),
    ((2, 64, 37, 7, 7), .1),
    ((0, 64, 37, 7, 3), .1),
    ((-1, 64, 37, 7, 3), .1),
    ((2, 64, 0, 7, 3), .1),
    ((1 << 20, 64, 1 << 20, 7, 3), .1),     # 2^40 pixels
    ((1 << 16, 64, 1 << 15, 7, 3), .1),     # 2^31 pixels
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
        assert library.pm_gconv_workspace_bytes(*sizes) == 0
    # (the pointers are never read: the sizes are refused first)
    code = library.pm_gconv_forward(
        256, 256, 256, 256, 256, *sizes, slope, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_gconv_forward' in library.pm_last_error()
    code = library.pm_gconv_backward(
        256, 256, 256, 256, 256, 256, *sizes, slope, 256, 1 << 40, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_gconv_backward' in library.pm_last_error()


@pytest.mark.parametrize('channels', oracle.CHANNELS)
def test_the_abi_refuses_null_pointers_and_a_small_workspace(channels):
    library = _lib.lib()
    for kernel in oracle.KERNELS:
        sizes = (2, channels, 37, kernel, 5)
        need = library.pm_gconv_workspace_bytes(*sizes)
        assert need >= 4 * (channels * channels * kernel + channels) \
            and need % 256 == 0
        # x, weight, bias and y; the residual (3) is optional
        for null in (0, 1, 2, 4):
            pointers = [256] * 5
            pointers[null] = None
            code = library.pm_gconv_forward(*pointers, *sizes, .1, None)
            assert code == _lib.PM_EINVAL
            assert b'pm_gconv_forward' in library.pm_last_error()
        # upstream, x, weight; one of gW and gb alone; gx (3) is optional
        for null in (0, 1, 2, 4, 5):
            pointers = [256] * 6
            pointers[null] = None
            code = library.pm_gconv_backward(
                *pointers, *sizes, .1, 256, need, None)
            assert code == _lib.PM_EINVAL
            assert b'pm_gconv_backward' in library.pm_last_error()
        code = library.pm_gconv_backward(
            *[256] * 6, *sizes, .1, None, need, None)
        assert code == _lib.PM_EINVAL
        code = library.pm_gconv_backward(
            *[256] * 6, *sizes, .1, 256, need - 1, None)
        assert code == _lib.PM_ENOMEM
        assert b'pm_gconv_backward' in library.pm_last_error()


def test_the_workspace_stays_modest_at_the_training_shape():
    """batch 64 x 64 frames: at most GC_GW_WORKGROUPS workgroups of gW, tiles
    x partials, so a layer's partials stay under 64 MB, and the split is the
    oracle's restatement of it"""
    library = _lib.lib()
    frames = 64
    for channels, rate in zip((256, 128, 64, 32), (8, 8, 2, 2)):
        frames *= rate
        for kernel in oracle.KERNELS:
            need = library.pm_gconv_workspace_bytes(
                64, channels, frames, kernel, 1)
            parts, _ = oracle.split(64, channels, frames)
            partial = 4 * (channels * channels * kernel + channels)
            assert parts * partial <= need < parts * partial + 256
            assert 0 < need <= 64 << 20
    assert frames == 16384


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
    promonet.model.hifigan = types.SimpleNamespace(
        Block=type('Block', (), dict(members)))
    return promonet


def test_patch_wraps_forward_once_and_keeps_the_original():
    promonet = stand_in()
    cls = promonet.model.hifigan.Block
    original = cls.forward
    promonet_amd.patch(promonet)
    assert cls.forward is not original and cls.forward.original is original
    # a CPU tensor goes to the original method
    assert cls().forward(torch.zeros(1, 32, 8)) == 'forward'
    promonet_amd.patch(promonet)
    assert cls.forward.original is original


def test_patch_leaves_a_class_without_forward_alone():
    promonet = stand_in(with_forward=False)
    promonet_amd.patch(promonet)
    assert not hasattr(promonet.model.hifigan.Block, 'forward')


def conv(channels, kernel, dilation=1, **kwargs):
    kwargs.setdefault('padding', (kernel - 1) // 2 * dilation)
    return torch.nn.utils.weight_norm(torch.nn.Conv1d(
        channels, channels, kernel, 1, dilation=dilation, **kwargs))


def reference_layout(channels=64, kernel=7, **changes):
    """The layers of the reference's Block; `changes` replaces c1{index},
    c2{index} or a{index}"""
    layout = types.SimpleNamespace(
        convs1=[conv(channels, kernel, d) for d in (1, 3, 5)],
        convs2=[conv(channels, kernel) for _ in range(3)],
        activations1=[torch.nn.LeakyReLU(.1) for _ in range(3)],
        activations2=[torch.nn.LeakyReLU(.1) for _ in range(3)])
    for key, value in changes.items():
        target = {'c1': layout.convs1, 'c2': layout.convs2,
                  'a': layout.activations1}[key[:-1]]
        target[int(key[-1])] = value
    return layout


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_only_the_reference_s_layer_layout_takes_the_device_path():
    layers = hifigan_train._block_layers(reference_layout())
    assert [(d1, s1, d2, s2) for _, d1, s1, _, d2, s2 in layers] == [
        (d, .1, 1, .1) for d in (1, 3, 5)]
    for changes in (
            {'c11': conv(64, 7, 2)},                    # another dilation
            {'c11': conv(64, 7, 3, padding=3)},         # not 'same'
            {'c11': conv(64, 3, 3)},                    # another kernel
            {'c20': conv(64, 7, bias=False)},
            {'c20': conv(64, 7, padding_mode='reflect')},
            {'c20': conv(64, 7, groups=2)},
            {'c20': torch.nn.Conv1d(64, 64, 7, padding=3)},
            {'c22': conv(32, 7)},
            {'a0': torch.nn.ReLU()},
            {'a1': torch.nn.LeakyReLU(0.)},
            {'a2': torch.nn.LeakyReLU(1.5)}):
        assert hifigan_train._block_layers(
            reference_layout(**changes)) is None, changes
    assert hifigan_train._block_layers(reference_layout(48, 7)) is None
    assert hifigan_train._block_layers(reference_layout(64, 5)) is None
    short = reference_layout()
    short.convs2 = short.convs2[:2]
    assert hifigan_train._block_layers(short) is None
    assert hifigan_train._block_layers(types.SimpleNamespace()) is None

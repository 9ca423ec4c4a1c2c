"""The conv stacks of the FARGAN discriminator without a GPU: the float64
oracle (tests/fdisc_oracle.py) against torch's conv2d and against the
reference's own run (tests/golden/fdisc.pt), the plan and the state_dict, the
conditions the GPU tests rely on, the planted defects their comparison must
reject, the size checks and `patch()`.
"""
import types
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.model import discriminator

import conv_checks
import fdisc_oracle as oracle
from conv_checks import close

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
NORM_SHAPES = [(16, 18, 3, 3), (16, 3, 3, 3), (1, 18, 3, 3)]


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'fdisc.pt')


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_layer_oracle_equals_conv2d_in_float64(name):
    _, _, _, _, dilation, activation = oracle.CASES[name]
    want = oracle.truth(name)
    _, y, gradients = oracle.reference_fp32(
        want['x'], want['weight'], want['bias'], dilation, activation,
        torch.float64, want['upstream'])
    assert close(want['forward'], y)
    for quantity, theirs in zip(oracle.QUANTITIES[1:], gradients):
        assert want[quantity].shape == theirs.shape
        assert close(want[quantity], theirs), quantity


@pytest.mark.parametrize('shape', NORM_SHAPES)
def test_the_weight_norm_oracle_equals_torch_in_float64(shape):
    generator = torch.Generator().manual_seed(1)
    g = (torch.rand(shape[0], 1, 1, 1, generator=generator) + .5).double()
    v = torch.randn(shape, generator=generator).double()
    upstream = torch.randn(shape, generator=generator).double()
    leaf_g, leaf_v = g.clone().requires_grad_(True), v.clone().requires_grad_(True)
    w = torch._weight_norm(leaf_v, leaf_g, 0)
    w.backward(upstream)
    assert close(oracle.weight_norm(g, v), w.detach())
    grad_g, grad_v = oracle.weight_norm_backward(upstream, g, v)
    assert grad_g.shape == g.shape
    assert close(grad_g, leaf_g.grad) and close(grad_v, leaf_v.grad)


def test_the_stack_oracle_equals_the_reference(golden):
    kept = golden['stacks'][0]
    assert kept['resolution'] == [64, 16, 64]
    parameters = [tuple(kept['parameters'][f'layers.{i}.1.{key}']
                        for key in ('weight_g', 'weight_v', 'bias'))
                  for i in range(6)]
    assert all(p.dtype == torch.float32 for triple in parameters
               for p in triple)
    logits, maps, saved = oracle.stack(
        kept['x'], parameters, kept['dilations'])
    assert kept['logits'].dtype == torch.float64
    assert close(logits, kept['logits'])
    for mine, theirs in zip(maps, kept['maps']):
        assert close(mine.flatten()[::golden['map_stride']], theirs)
    grad_x, gradients = oracle.stack_backward(
        saved, parameters, oracle.coefficients(*kept['x'].shape[::2],
                                               kept['x'].shape[3]))
    assert close(grad_x, kept['gradient_x'])
    for i, triple in enumerate(gradients):
        for key, mine in zip(('weight_g', 'weight_v', 'bias'), triple):
            step = golden['gradient_stride'] if key == 'weight_v' else 1
            assert close(mine.flatten()[::step],
                         kept['gradients'][f'layers.{i}.1.{key}']), (i, key)


###############################################################################
# The plan and the state_dict
###############################################################################


@pytest.mark.parametrize('n_fft', discriminator.RESOLUTIONS)
def test_the_plan_is_the_reference_s(golden, n_fft):
    plan = discriminator.magfree_plan(n_fft)
    recorded = golden['plans'][n_fft]
    assert len(plan) == len(recorded) == 6
    for (stride, dilation, _, _), entry in zip(plan, recorded):
        assert entry == [[stride, 1], [dilation, 1], [dilation, 1]]
    # the shapes of the checkpoint follow from the plan's channels
    shapes = dict(zip(golden['keys'][n_fft], golden['shapes'][n_fft]))
    bins = n_fft // 2 + 1
    assert shapes.pop('filterbank') == [bins, bins]
    for index, (_, _, channels, out_channels) in enumerate(plan):
        assert shapes.pop(f'layers.{index}.1.bias') == [out_channels]
        assert shapes.pop(f'layers.{index}.1.weight_g') == \
            [out_channels, 1, 1, 1]
        assert shapes.pop(f'layers.{index}.1.weight_v') == \
            [out_channels, channels + 2, 3, 3]
    assert not shapes


def test_the_plan_refuses_other_sizes():
    for n_fft in (32, 96, 4096, 64.5):
        with pytest.raises(ValueError):
            discriminator.magfree_plan(n_fft)


def test_the_module_has_the_reference_s_keys_and_shapes(golden):
    module = discriminator.DiscriminatorMagFree([64, 16, 64])
    state = module.state_dict()
    assert list(state) == golden['keys'][64]
    assert [list(v.shape) for v in state.values()] == golden['shapes'][64]
    assert not module.filterbank.requires_grad
    # the reference's checkpoint loads
    kept = golden['stacks'][0]['parameters']
    module.load_state_dict(
        dict(kept, filterbank=torch.ones_like(state['filterbank'])))
    assert torch.equal(module.layers[3][1].weight_v,
                       kept['layers.3.1.weight_v'])


@pytest.mark.parametrize('n_fft', discriminator.RESOLUTIONS[1:])
def test_the_module_refuses_the_strided_resolutions(golden, n_fft):
    """At 128 ... 2048 the reference's layers halve the frequency axis and
    widen to 32 ... 256 channels: no kernel, so an error"""
    assert any(entry[0] == [2, 1] for entry in golden['plans'][n_fft])
    with pytest.raises(ValueError, match='stride'):
        discriminator.DiscriminatorMagFree([n_fft, n_fft // 4, n_fft])


###############################################################################
# What the GPU tests rely on
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_fragile_share_is_small(name):
    conv_checks.the_fragile_share_is_small(oracle, name)


def test_the_large_case_reaches_past_one_workgroup_and_one_partial():
    channels, _, bins, frames, _, _ = oracle.CASES['large']
    pixels = oracle.BATCH * bins * frames
    assert pixels > oracle.CONSTANTS['FD_CONV_PIXELS']
    assert oracle.CONSTANTS['FD_GW_CHUNK'] < pixels < \
        2 * oracle.CONSTANTS['FD_GW_CHUNK']
    # two weight-gradient workgroups of `span` pixels, a quarter a wave: the
    # last wave ends in a step of fewer than four pixels
    span = (-(-pixels // 2) + 15) // 16 * 16
    assert 0 < pixels - span - 3 * (span // 4) < span // 4
    assert (pixels - span - 3 * (span // 4)) % 4
    assert pixels % 16
    # and the partials of the workspace say so
    need = _lib.lib().pm_fdisc_workspace_bytes(
        oracle.BATCH, channels, 16, bins, frames)
    one = _lib.lib().pm_fdisc_workspace_bytes(1, channels, 16, 8, 8)
    assert need > one


@pytest.mark.parametrize('name', NAMES)
def test_the_gates_come_from_the_reference_arithmetic_in_fp32(name):
    conv_checks.the_gates_come_from_the_reference_arithmetic_in_fp32(
        oracle, name)


###############################################################################
# Planted defects: the comparison of the GPU tests (the shapes and the four
# figures against the gates) rejects each of them in every case it can touch
###############################################################################

DILATED = ['d2', 'd4', 'd8-one-frame', 'd16', 'large']
RELU = [name for name in NAMES if oracle.CASES[name][5] == 'relu']
APPLIES = {
    'angle': NAMES,
    'swapped': NAMES,
    'embedding_unpadded_frequency': NAMES,
    'embedding_unpadded_time': NAMES,
    'dilation_on_time': DILATED,
    'padding_one': DILATED,
    'taps_transposed': NAMES,
    'relu_mask_from_input': RELU,
    'sigmoid_gradient_left_out': ['last'],
    'embedding_weight_gradient_dropped': NAMES,
}


def accepted(name, defect):
    """Would the GPU tests pass an implementation with this defect?"""
    form = oracle.CASES[name][4:]
    return conv_checks.accepted(
        oracle, name, lambda *inputs: oracle.layer(*inputs, *form, defect),
        lambda *inputs: oracle.layer_backward(*inputs, *form, defect))


def test_the_defects_are_all_listed():
    assert set(APPLIES) | {'norm_whole_tensor'} == set(oracle.DEFECTS)


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_itself_is_accepted(name):
    assert accepted(name, None)


@pytest.mark.parametrize(
    'defect,name',
    [(defect, name) for defect in APPLIES for name in APPLIES[defect]])
def test_a_planted_defect_is_rejected(defect, name):
    assert not accepted(name, defect)


@pytest.mark.parametrize('shape', NORM_SHAPES[:2])
def test_a_norm_over_the_whole_tensor_is_rejected(shape):
    generator = torch.Generator().manual_seed(shape[0] * 100 + shape[1])
    g = torch.rand(shape[0], 1, 1, 1, generator=generator) + .5
    v = torch.randn(shape, generator=generator)
    upstream = torch.randn(shape, generator=generator)
    want = (oracle.weight_norm(g, v),) + \
        oracle.weight_norm_backward(upstream, g, v)
    for defect, verdict in ((None, True), ('norm_whole_tensor', False)):
        got = (oracle.weight_norm(g, v, defect),) + \
            oracle.weight_norm_backward(upstream, g, v, defect)
        assert verdict == all(
            oracle.figure(mine, theirs) < limit for mine, theirs, limit in
            zip(got, want, oracle.WEIGHT_NORM_GATES))


###############################################################################
# Sizes: ValueError from Python, PM_EINVAL from the ABI, no device needed
###############################################################################


def arguments(channels=16, out_channels=16, bins=9, frames=5):
    return (torch.zeros(2, channels, bins, frames),
            torch.zeros(out_channels, channels + 2, 3, 3),
            torch.zeros(out_channels))


BAD = [
    (lambda x, w, b: (x[0], w, b), {}),                        # not 4-D
    (lambda x, w, b: (x[:, :8], w[:, :10], b), {}),            # C = 8
    (lambda x, w, b: (x, w[:8], b[:8]), {}),                   # O = 8
    (lambda x, w, b: (x, w[:, :16], b), {}),                   # no embedding
    (lambda x, w, b: (x, w[..., :2], b), {}),                  # not 3 x 3
    (lambda x, w, b: (x, w, b[:1]), {}),                       # bias
    (lambda x, w, b: (x[:, :, :0], w, b), {}),                 # empty
    (lambda x, w, b: (x.long(), w, b), {}),                    # not float
    (lambda x, w, b: (x, w, b), {'dilation': 3}),
    (lambda x, w, b: (x, w, b), {'dilation': (2, 2)}),
    (lambda x, w, b: (x, w, b), {'activation': 'tanh'}),
    (lambda x, w, b: (x, w, b), {'table': torch.zeros(8, 2)}),
]


@pytest.mark.parametrize('change,keywords', BAD)
def test_bad_arguments_raise_before_any_device_work(change, keywords):
    with pytest.raises(ValueError):
        discriminator.frequency_conv(*change(*arguments()), **keywords)


def test_one_channel_on_both_sides_is_refused():
    with pytest.raises(ValueError):
        discriminator.frequency_conv(*arguments(1, 1))
    with pytest.raises(ValueError):
        discriminator.weight_norm(torch.zeros(4), torch.zeros(3, 2))


def test_good_sizes_on_a_cpu_tensor_say_that_there_is_no_fallback():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.frequency_conv(*arguments())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.weight_norm(torch.ones(16, 1, 1, 1),
                                  torch.ones(16, 18, 3, 3))


ABI_BAD = [
    # batch, channels, out_channels, bins, frames, dilation, activation
    (2, 8, 16, 33, 7, 1, 1),
    (2, 16, 8, 33, 7, 1, 1),
    (2, 1, 1, 33, 7, 1, 1),
    (2, 16, 16, 33, 7, 3, 1),
    (2, 16, 16, 33, 7, 32, 1),
    (2, 16, 16, 33, 7, 0, 1),
    (0, 16, 16, 33, 7, 1, 1),
    (2, 16, 16, 0, 7, 1, 1),
    (2, 16, 16, 33, 0, 1, 1),
    (2, 16, 16, 33, 7, 1, 3),
    (2, 16, 16, 33, 7, 1, -1),
    (1 << 20, 16, 16, 1 << 10, 1 << 10, 1, 1),      # the grid
]


@pytest.mark.parametrize('sizes', ABI_BAD)
def test_the_abi_refuses_bad_sizes_on_the_host(sizes):
    library = _lib.lib()
    if sizes[5] == 1 and 0 <= sizes[6] < 3:
        assert library.pm_fdisc_workspace_bytes(*sizes[:5]) == 0
    # (the pointers are never read: the sizes are refused first)
    code = library.pm_fdisc_conv_forward(
        256, 256, 256, 256, 256, *sizes, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_conv_forward' in library.pm_last_error()
    code = library.pm_fdisc_conv_backward(
        256, 256, 256, 256, 256, 256, 256, 256, *sizes, 256, 1 << 40, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_conv_backward' in library.pm_last_error()


def test_the_abi_refuses_null_pointers_and_a_small_workspace():
    library = _lib.lib()
    sizes = (2, 16, 16, 33, 7, 1, 1)
    need = library.pm_fdisc_workspace_bytes(*sizes[:5])
    assert need >= 256 and need % 256 == 0
    code = library.pm_fdisc_conv_forward(
        256, 256, None, 256, 256, *sizes, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_conv_forward' in library.pm_last_error()
    code = library.pm_fdisc_conv_backward(
        256, 256, 256, 256, 256, 256, 256, None, *sizes, 256, need, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_conv_backward' in library.pm_last_error()
    code = library.pm_fdisc_conv_backward(
        256, 256, 256, 256, 256, 256, 256, 256, *sizes, 256, need - 1, None)
    assert code == _lib.PM_ENOMEM
    assert b'pm_fdisc_conv_backward' in library.pm_last_error()


@pytest.mark.parametrize('sizes', [(0, 162), (16, 0), (1 << 16, 162)])
def test_the_weight_norm_entries_refuse_bad_sizes(sizes):
    library = _lib.lib()
    code = library.pm_fdisc_weight_norm_forward(256, 256, 256, *sizes, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_weight_norm_forward' in library.pm_last_error()
    code = library.pm_fdisc_weight_norm_backward(
        256, 256, 256, 256, 256, *sizes, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_weight_norm_backward' in library.pm_last_error()
    assert library.pm_fdisc_weight_norm_forward(
        None, 256, 256, 16, 162, None) == _lib.PM_EINVAL


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
        SpecDiscriminatorBase=type('SpecDiscriminatorBase', (), members))
    return promonet


def test_patch_wraps_forward_once_and_keeps_the_original():
    promonet = stand_in()
    base = promonet.model.discriminator.SpecDiscriminatorBase
    original = base.forward
    promonet_amd.patch(promonet)
    assert base.forward is not original and base.forward.original is original
    # a CPU tensor goes to the original method
    assert base().forward(torch.zeros(1, 1, 8)) == 'forward'
    promonet_amd.patch(promonet)
    assert base.forward.original is original


def test_patch_leaves_a_class_without_forward_alone():
    promonet = stand_in(with_forward=False)
    base = promonet.model.discriminator.SpecDiscriminatorBase
    promonet_amd.patch(promonet)
    assert not hasattr(base, 'forward')
    assert hasattr(base.spectrogram, 'original')
